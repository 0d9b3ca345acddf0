"""CPU tests of the per-cell sources (include/mpdata_hip.h 3p): the numpy model of tests/cell_add_model.py against a
scalar triple loop and against what the definition implies -- c = 0 and s = 0, a single non-zero cell, dsum under the
clip, the merge property of level windows --, the plan model's rules, and the interface (header, ctypes, Fortran, Python
names, the argument checks that need no device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cell_add_model as CM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_cell_add_device", "mpdata_plan_cell_add", "mpdata_plan_cell_add_f32", "mpdata_cell_add_device",
         "mpdata_cell_add_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


# ---- the model against the definition
@pytest.mark.parametrize("mode", [CM.ADD, CM.CLIP], ids=["add", "clip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, mode):
    """c = 0.1 is no fp32 number: the loop rounds it once, then multiplies"""
    n, nx, nz, T = 3, 4, 6, 2
    nzm = nz - 1
    R = np.dtype(dtype).type
    f = field(n, nx, nz, T, dtype, 11)
    s = CM.make_s(n, nx, nz, T, dtype, 13)
    assert (s < 0).any() and (s > 0).any() and (f < 0).any() and (f > 0).any()
    c = 0.1
    new, dsum = CM.cell_add(f, s, c, mode)
    want, wd = np.array(f, order="F"), np.zeros((n, nzm, T), dtype)
    cf = R(c)
    for t in range(T):
        for b in range(n):
            for k in range(nzm):
                a = R(0)
                for i in range(nx):
                    p = R(cf * s[b, i, k, t])
                    g = R(f[b, i + 3, k, t] + p)
                    if mode == CM.CLIP:
                        g = max(R(0), g)
                    a = R(a + R(g - f[b, i + 3, k, t]))
                    want[b, i + 3, k, t] = g
                wd[b, k, t] = a
    assert np.array_equal(CM.bits(new), CM.bits(want)) and np.array_equal(CM.bits(dsum), CM.bits(wd))
    assert not np.array_equal(new, f)
    if dtype == np.float32:
        # the single rounding is visible: the product formed in double and rounded afterwards differs somewhere
        twice = (np.float64(c) * s.astype(np.float64)).astype(np.float32)
        assert not np.array_equal(twice, np.float32(c) * s)
    # one tracer with and without the axis
    n1, d1 = CM.cell_add(np.asfortranarray(f[..., 1]), np.asfortranarray(s[..., 1]), c, mode)
    assert np.array_equal(CM.bits(n1), CM.bits(new[..., 1])) and np.array_equal(CM.bits(d1), CM.bits(dsum[..., 1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_c_zero_and_s_zero_keep_every_bit(dtype):
    """... except -0 + +0 = +0; dsum = +0"""
    n, nx, nz = 3, 4, 9
    f = field(n, nx, nz, 1, dtype, 5)
    f[0, 4, 2] = 0.0
    f[1, 5, 3] = -0.0
    s = CM.make_s(n, nx, nz, None, dtype, 6)
    s[1, 2, 3] = 0.25                                        # (0 * a negative s is -0, and -0 + -0 stays -0)
    for new, dsum in (CM.cell_add(f, s, 0.0), CM.cell_add(f, np.zeros_like(s), 0.75)):
        want = np.array(f)
        want[1, 5, 3] = 0.0                                  # -0 + +0 = +0
        assert np.array_equal(CM.bits(new), CM.bits(want))
        assert not np.any(dsum) and not np.any(np.signbit(dsum))
    # a -0 stays where the product is -0 too: c * s = 0.75 * -0
    z = np.full((1, 7, 3), -0.0, dtype, order="F")
    new, dsum = CM.cell_add(z, np.full((1, 1, 3), -0.0, dtype, order="F"), 0.75)
    assert np.all(np.signbit(new)) and not np.any(new)
    assert not np.any(dsum) and not np.any(np.signbit(dsum))  # a sum that starts at +0 never becomes -0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_single_cell_changes_that_cell_alone(dtype):
    n, nx, nz, T = 2, 3, 7, 2
    f = field(n, nx, nz, T, dtype, 8)
    f[1, 4, 3, 1] = 8.0
    s = np.zeros((n, nx, nz - 1, T), dtype, order="F")
    s[1, 1, 3, 1] = 4.0
    new, dsum = CM.cell_add(f, s, 0.5)
    want = np.array(f)
    want[1, 4, 3, 1] = 10.0
    assert np.array_equal(CM.bits(new), CM.bits(want))
    assert dsum[1, 3, 1] == 2.0 and np.count_nonzero(dsum) == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dsum_under_clip_is_the_applied_change(dtype):
    n, nx, nz = 2, 5, 6
    f = field(n, nx, nz, 1, dtype, 9)
    s = CM.make_s(n, nx, nz, None, dtype, 10)
    c = 0.75
    frac = CM.clipped_fraction(f, s, c)
    assert 0.1 <= frac <= 0.9
    new, dsum = CM.cell_add(f, s, c, CM.CLIP)
    assert np.all(new[:, 3:nx + 3] >= 0) and np.array_equal(CM.bits(new[:, :3]), CM.bits(f[:, :3]))
    applied = np.zeros_like(dsum)
    asked = np.zeros_like(dsum)
    for i in range(nx):
        applied = applied + (new[:, i + 3] - f[:, i + 3])
        asked = asked + np.dtype(dtype).type(c) * s[:, i]
    assert np.array_equal(CM.bits(dsum), CM.bits(applied))
    assert not np.array_equal(dsum, asked)
    # without the clip the two differ by the rounding of g - f at most: here they agree to a few ulp of the operands
    _, d0 = CM.cell_add(f, s, c, CM.ADD)
    assert np.allclose(d0, asked, rtol=0, atol=nx * 4 * np.finfo(dtype).eps)


@pytest.mark.parametrize("mode", [CM.ADD, CM.CLIP], ids=["add", "clip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 250, 300, 1000])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype, mode):
    """the operator on every level window as a problem of its own (s of the tall levels it stands for), owned levels
    merged == the operator on the tall column, bit for bit; dsum from each level's owner.  The geometry is the library's."""
    n, nx, T = 2, 3, 2
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    s = CM.make_s(n, nx, nz, T, dtype, 23)
    want, want_d = CM.cell_add(f, s, 0.75, mode)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_d = np.full_like(want, np.nan), np.full_like(want_d, np.nan)
    got[:, :3], got[:, nx + 3:] = f[:, :3], f[:, nx + 3:]
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, d = CM.cell_add(np.asfortranarray(f[:, :, lev]), np.asfortranarray(s[:, :, lev]), 0.75, mode)
        assert k0 + 1 <= own0 <= own1 <= k0 + nz_w - 1
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, 3:nx + 3, own], got_d[:, own] = new[:, 3:nx + 3, loc], d[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)                            # every tall level owned exactly once
    assert np.array_equal(CM.bits(got), CM.bits(want)) and np.array_equal(CM.bits(got_d), CM.bits(want_d))
    assert not np.array_equal(want, f)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = CM.PlanModelCellAdd(oracle, *shape, T, dtype)
    return m, CM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    s = CM.make_s(5, 8, 6, 2, np.float64, 6)
    assert m.cell_add(s) == PM.ESTATE                                       # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.cell_add(s, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.cell_add(s, first=1, ntr=2) == PM.EINVAL and m.cell_add(s, first=-1, ntr=1) == PM.EINVAL
    assert m.cell_add(s, first=0, ntr=0) == PM.EINVAL
    assert m.cell_add(None) == PM.EINVAL
    assert m.cell_add(s, mode=2) == PM.EINVAL and m.cell_add(s, mode=-1) == PM.EINVAL
    assert m.cell_add(s, eb=4) == PM.ESTATE                                 # a host form of the other precision
    assert m.cell_add(None, eb=4) == PM.EINVAL and m.cell_add(s, mode=2, eb=4) == PM.EINVAL    # the NULL and the mode come first
    m.multi = True
    assert m.cell_add(s) == PM.EUNSUPPORTED and m.cell_add(s, sl0=0, n=0) == PM.EINVAL
    assert m.cell_add(None) == PM.EUNSUPPORTED                              # the handle comes before the NULL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(CM.bits(m.a[k]), CM.bits(v)), k
    d = m.cell_add(s, 0.75, CM.CLIP)
    assert d.shape == (5, 5, 2) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(CM.bits(m.a["f"][:, :3]), CM.bits(keep["f"][:, :3]))            # halo columns keep every bit
    assert np.array_equal(CM.bits(m.a["f"][:, 11:]), CM.bits(keep["f"][:, 11:]))
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(CM.bits(m.a[k]), CM.bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_cell_add_is_export_change_import(oracle, boundary):
    """the call on a block and a tracer = export of the block, the operator, import; on a PERIODIC model the halos of the
    next read-back are wrapped copies of the NEW interior"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    s = CM.make_s(3, 8, 6, None, np.float64, 7)
    d = a.cell_add(s, 0.75, CM.CLIP, sl0=1, n=3, first=1, ntr=1)
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new, d2 = CM.cell_add(exp[..., 0], s, 0.75, CM.CLIP)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    assert np.array_equal(CM.bits(d[..., 0]), CM.bits(d2))
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(CM.bits(ea[k]), CM.bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(CM.bits(e), CM.bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(CM.bits(e[1:4, 3:11, :, 1]), CM.bits(new[:, 3:11]))          # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(CM.bits(ea[k]), CM.bits(eb[k])), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.cell_add) and callable(mpdata.Plan.cell_add) and callable(mpdata.Plan.cell_add_host)
    for nm in ("cell_add", "cell_add_shapes", "CELL_ADD", "CELL_ADD_CLIP"):
        assert nm in mpdata.__all__, nm
    assert (mpdata.CELL_ADD, mpdata.CELL_ADD_CLIP) == (0, 1) == (CM.ADD, CM.CLIP)
    assert mpdata.cell_add_shapes(5, 3, 8) == {"s": (7, 3, 5), "dsum": (7, 5)}
    assert mpdata.cell_add_shapes(5, 3, 8, 2) == {"s": (2, 7, 3, 5), "dsum": (2, 7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3p." in hdr
    sec = hdr.split("---- 3p.")[1].split("---- 4.")[0]
    for word in ("s", "c", "dsum", "MPDATA_CELL_ADD", "MPDATA_CELL_ADD_CLIP"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_CELL_ADD 0\b", sec) and re.search(r"#define MPDATA_CELL_ADD_CLIP 1\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels only" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec
    assert hdr.index("---- 3o.") < hdr.index("---- 3p.") < hdr.index("---- 4.")


def test_library_exports_and_ctypes_agree_with_the_header(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*", ctypes.c_double: "double", ctypes.c_float: "float"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)
    # the factor: a double in the device form and the fp64 forms, a float in the fp32 forms
    assert _c_params(hdr, "mpdata_plan_cell_add_device")[4] == "double c"
    assert _c_params(hdr, "mpdata_plan_cell_add_f32")[4] == "float c" and _c_params(hdr, "mpdata_cell_add_f32_device")[8] == "float c"


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value; c is real(c_double), value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_cell_add_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_cell_add_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_cell_add_device")
    cargs = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert fargs == cargs, (fargs, cargs)
    decl = {}
    for line in m.group(2).splitlines():
        d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\)|real\(c_double\))\s*,\s*value\s*::\s*(.*)", line)
        if d:
            for a in d.group(2).split(","):
                decl[a.strip()] = d.group(1)
    for p, a in zip(params, cargs):
        want = ("type(c_ptr)" if "*" in p else "integer(c_int64_t)" if p.startswith("int64_t ") else
                "real(c_double)" if p.startswith("double ") else "integer(c_int)")
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert decl["c"] == "real(c_double)"
    assert "c_double" in re.search(r"import ::(.*)", m.group(2)).group(1)
    assert re.search(r"public ::.*\bmpdata_plan_cell_add_device_c\b", f90)
    assert re.search(r"MPDATA_CELL_ADD = 0, MPDATA_CELL_ADD_CLIP = 1", f90)
    assert "MPDATA_C_PLAN_CELL_ADD" not in f90 and "MPDATA_C_CELL_ADD" not in f90        # no per-precision macro
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "cell_add_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_cell_add_device, L.mpdata_cell_add_f32_device):
        assert fn(4, 0, 6, 1, 0, 4, one, one, 1.0, 0, None, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, one, one, 1.0, 0, None, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 4, one, one, 1.0, 0, None, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, one, one, 1.0, 0, None, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, one, one, 1.0, 0, None, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, None, one, 1.0, 0, None, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, one, None, 1.0, 0, None, None) == mpdata.EINVAL and b"null s" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, None, None, 1.0, 7, None, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, one, None, 1.0, 7, None, None) == mpdata.EINVAL and b"null s" in L.mpdata_last_error()
        for mode in (2, -1, 7):
            assert fn(4, 5, 6, 1, 0, 4, one, one, 1.0, mode, None, None) == mpdata.EINVAL and b"unknown mode" in L.mpdata_last_error()
        assert fn(4, 5, 1, 1, 0, 4, None, None, 1.0, 7, None, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert L.mpdata_plan_cell_add_device(None, 0, 1, one, 1.0, 0, None, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error()
    assert L.mpdata_plan_cell_add(None, 0, 1, one, 1.0, 0, None) == mpdata.EINVAL
    assert L.mpdata_plan_cell_add_f32(None, 0, 1, one, 1.0, 0, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_cell_add_device(one, sl0, n, one, 1.0, 0, None, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_cell_add_device(one, 0, 0, None, 1.0, 9, None, 0, 1) == mpdata.EINVAL
    assert b"null s" not in L.mpdata_last_error() and b"unknown mode" not in L.mpdata_last_error()   # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_cell_add.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel; the LDS of the plan-layout kernel is dynamic, its budget a constant of
    the file: 40 KiB at most, four workgroups per CU"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_cell_add.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    # f64 plain and windowed, f32 plain in pairs, plain in reals and windowed; each with and without dsum
    assert len(re.findall(r"Function Name: \S*wm_cell_add_kernel", txt)) == 10
    assert len(re.findall(r"Function Name: \S*ref_cell_add_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 12 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}      # (static: none; the dynamic size below)
    src = open(os.path.join(csrc, "mpdata_cell_add.hip")).read()
    walk = open(os.path.join(csrc, "mpdata_wm_walk.h")).read()
    m = re.search(r"constexpr int LDS_ELEMS = (\d+);", walk)                               # (the one statement of the limit)
    assert m and int(m.group(1)) * 8 <= 40 * 1024
    assert "col_groups_tiled(j, b.sel, wg, LDS_ELEMS," in src and "g->lds_e <= budget" in walk     # the launch refuses more
