"""CPU tests of the relaxation to a level profile (include/mpdata_hip.h 3r): the numpy model of tests/relax_model.py
against a scalar triple loop and against what the definition implies -- c = 0 levels, c = 1, the target that is the mean,
the single rounding of the division, the merge property of level windows --, the plan model's rules, and the interface
(header, ctypes, Fortran, Python names, the argument checks that need no device, the compiler's resource report).  No test
here needs a GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import relax_model as RM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_relax_device", "mpdata_plan_relax", "mpdata_plan_relax_f32", "mpdata_relax_device", "mpdata_relax_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


# ---- the model against the definition
@pytest.mark.parametrize("mode", ["mean", "target"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, mode):
    n, nx, nz, T = 3, 5, 7, 2
    nzm = nz - 1
    R = np.dtype(dtype).type
    f = field(n, nx, nz, T, dtype, 11)
    c = RM.make_c(n, nz, dtype, 12)
    assert (c == 0).any() and (c > 0).any() and (f < 0).any() and (f > 0).any()
    tgt = RM.make_target(n, nz, T, dtype, 13) if mode == "target" else None
    new, mean = RM.relax(f, c, tgt)
    want, wm = np.array(f, order="F"), np.zeros((n, nzm, T), dtype)
    for t in range(T):
        for b in range(n):
            for k in range(nzm):
                if tgt is None:
                    s = R(0)
                    for i in range(nx):
                        s = R(s + f[b, i + 3, k, t])
                    m = R(s / R(nx))
                else:
                    m = tgt[b, k, t]
                wm[b, k, t] = m
                if c[b, k] == 0:
                    continue
                for i in range(nx):
                    d = R(f[b, i + 3, k, t] - m)
                    p = R(c[b, k] * d)
                    want[b, i + 3, k, t] = R(f[b, i + 3, k, t] - p)
    assert np.array_equal(RM.bits(new), RM.bits(want)) and np.array_equal(RM.bits(mean), RM.bits(wm))
    assert not np.array_equal(new, f)
    # one tracer with and without the axis
    t1 = None if tgt is None else np.asfortranarray(tgt[..., 1])
    n1, m1 = RM.relax(np.asfortranarray(f[..., 1]), c, t1)
    assert np.array_equal(RM.bits(n1), RM.bits(new[..., 1])) and np.array_equal(RM.bits(m1), RM.bits(mean[..., 1]))


@pytest.mark.parametrize("mode", ["mean", "target"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_c_zero_levels_keep_every_bit(dtype, mode):
    """... -0.0 and negative values included, for c = +0 and c = -0; mean is written all the same"""
    n, nx, nz = 3, 4, 9
    f = field(n, nx, nz, 1, dtype, 5)
    f[0, 4, 2] = 0.0
    f[1, 5, 3] = -0.0
    f[2, 3, 1] = -0.25
    c = RM.make_c(n, nz, dtype, 6)
    c[1, 3] = -0.0
    zero = c == 0
    assert zero[1, 3] and zero[0, 2] and zero[2, 1] and not zero.all()
    tgt = RM.make_target(n, nz, None, dtype, 7) if mode == "target" else None
    new, mean = RM.relax(f, c, tgt)
    for b, k in zip(*np.nonzero(zero)):
        assert np.array_equal(RM.bits(new[b, :, k]), RM.bits(f[b, :, k])), (b, k)
    assert np.signbit(new[1, 5, 3]) and new[2, 3, 1] == dtype(-0.25)
    for b, k in zip(*np.nonzero(~zero)):
        assert not np.array_equal(RM.bits(new[b, 3:nx + 3, k]), RM.bits(f[b, 3:nx + 3, k])), (b, k)
    assert np.all(np.isfinite(mean)) and np.count_nonzero(mean) > mean.size // 2
    if tgt is not None:
        assert np.array_equal(RM.bits(mean), RM.bits(tgt))
    # the whole of c zero: f keeps every bit
    new0, mean0 = RM.relax(f, np.zeros_like(c), tgt)
    assert np.array_equal(RM.bits(new0), RM.bits(f)) and np.array_equal(RM.bits(mean0), RM.bits(mean))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_c_one_gives_the_mean_up_to_the_stated_roundings(dtype):
    """c = 1: f - 1 * (f - m) with d = f - m rounded, then f - d rounded -- m only up to those; the formula is asserted"""
    n, nx, nz = 2, 6, 5
    f = field(n, nx, nz, 1, dtype, 15)
    f[:, :, 1] += dtype(1000.0)                              # (a level where f - m loses bits)
    c = np.ones((n, nz - 1), dtype, order="F")
    new, mean = RM.relax(f, c)
    ci = f[:, 3:nx + 3]
    d = ci - mean[:, None]
    assert np.array_equal(RM.bits(new[:, 3:nx + 3]), RM.bits(ci - d))
    eps = np.finfo(dtype).eps
    assert np.all(np.abs(new[:, 3:nx + 3] - mean[:, None]) <= 2 * eps * np.maximum(np.abs(ci), np.abs(mean[:, None])))
    assert np.array_equal(RM.bits(new[:, :3]), RM.bits(f[:, :3])) and np.array_equal(RM.bits(new[:, nx + 3:]), RM.bits(f[:, nx + 3:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_target_equal_to_the_mean_reproduces_mean_mode(dtype):
    n, nx, nz, T = 3, 7, 8, 2
    f = field(n, nx, nz, T, dtype, 17)
    c = RM.make_c(n, nz, dtype, 18)
    new, mean = RM.relax(f, c)
    new2, mean2 = RM.relax(f, c, mean)
    assert np.array_equal(RM.bits(new), RM.bits(new2)) and np.array_equal(RM.bits(mean), RM.bits(mean2))


def _nearest(q, m, dtype):
    """m is a floating-point number of dtype nearest to the rational q"""
    e = abs(Fraction(float(m)) - q)
    return all(e <= abs(Fraction(float(np.nextafter(m, dtype(s) * np.inf))) - q) for s in (-1, 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_division_is_rounded_once(dtype):
    """m is the number of the plan's precision NEAREST to the exact quotient of the rounded sum and nx, for every element.
    Witnesses, asserted on the inputs: elements where the sum times the rounded reciprocal of nx differs, and (fp32)
    elements where the mean formed in double throughout and rounded at the end differs.  float(double(s) / nx), the
    fp32 sum divided in double and rounded again, is NO witness: a quotient of two 24-bit numbers formed in 53 bits and
    rounded to 24 is the correctly rounded quotient (53 >= 2 * 24 + 2), so no such element exists; the test asserts that
    equality instead, as a second check of numpy's division."""
    n, nx, nz = 40, 7, 6
    f = field(n, nx, nz, 1, dtype, 19)
    c = np.ones((n, nz - 1), dtype, order="F")
    _, mean = RM.relax(f, c)
    s = np.zeros_like(mean)
    for i in range(nx):
        s = s + f[:, i + 3]
    assert s.dtype == dtype
    for b in range(n):
        for k in range(nz - 1):
            assert _nearest(Fraction(float(s[b, k])) / nx, mean[b, k], dtype), (b, k)
    recip = s * (dtype(1) / dtype(nx))
    assert recip.dtype == dtype and np.any(RM.bits(recip) != RM.bits(mean))
    if dtype == np.float32:
        via_double = (s.astype(np.float64) / np.float64(nx)).astype(np.float32)
        assert np.array_equal(RM.bits(via_double), RM.bits(mean))
        all_double = (f[:, 3:nx + 3].astype(np.float64).sum(axis=1) / nx).astype(np.float32)
        assert np.any(RM.bits(all_double) != RM.bits(mean))


@pytest.mark.parametrize("mode", ["mean", "target"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 250, 300, 1000])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype, mode):
    """the operator on every level window as a problem of its own (c and the target of the tall levels it stands for),
    owned levels merged == the operator on the tall column, bit for bit; mean from each level's owner.  The geometry is
    the library's."""
    n, nx, T = 2, 3, 2
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    c = RM.make_c(n, nz, dtype, 22)
    tgt = RM.make_target(n, nz, T, dtype, 23) if mode == "target" else None
    want, want_m = RM.relax(f, c, tgt)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_m = np.full_like(want, np.nan), np.full_like(want_m, np.nan)
    got[:, :3], got[:, nx + 3:] = f[:, :3], f[:, nx + 3:]
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, m = RM.relax(np.asfortranarray(f[:, :, lev]), np.asfortranarray(c[:, lev]),
                          None if tgt is None else np.asfortranarray(tgt[:, lev]))
        assert k0 + 1 <= own0 <= own1 <= k0 + nz_w - 1
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, 3:nx + 3, own], got_m[:, own] = new[:, 3:nx + 3, loc], m[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)                            # every tall level owned exactly once
    assert np.array_equal(RM.bits(got), RM.bits(want)) and np.array_equal(RM.bits(got_m), RM.bits(want_m))
    assert not np.array_equal(want, f)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = RM.PlanModelRelax(oracle, *shape, T, dtype)
    return m, RM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    c = RM.make_c(5, 6, np.float64, 6)
    assert m.relax(c) == PM.ESTATE                                          # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.relax(c, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.relax(c, first=1, ntr=2) == PM.EINVAL and m.relax(c, first=-1, ntr=1) == PM.EINVAL
    assert m.relax(c, first=0, ntr=0) == PM.EINVAL
    assert m.relax(None) == PM.EINVAL
    assert m.relax(c, eb=4) == PM.ESTATE                                    # a host form of the other precision
    assert m.relax(None, eb=4) == PM.EINVAL                                 # the NULL comes first
    m.multi = True
    assert m.relax(c) == PM.EUNSUPPORTED and m.relax(c, sl0=0, n=0) == PM.EINVAL
    assert m.relax(None) == PM.EUNSUPPORTED                                 # the handle comes before the NULL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(RM.bits(m.a[k]), RM.bits(v)), k
    mean = m.relax(c)
    assert mean.shape == (5, 5, 2) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(RM.bits(m.a["f"][:, :3]), RM.bits(keep["f"][:, :3]))            # halo columns keep every bit
    assert np.array_equal(RM.bits(m.a["f"][:, 11:]), RM.bits(keep["f"][:, 11:]))
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(RM.bits(m.a[k]), RM.bits(keep[k])), k


@pytest.mark.parametrize("mode", ["mean", "target"])
@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_relax_is_export_change_import(oracle, boundary, mode):
    """the call on a block and a tracer = export of the block, the operator, import; on a PERIODIC model the halos of the
    next read-back are wrapped copies of the NEW interior"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    c = RM.make_c(3, 6, np.float64, 7)
    tgt = RM.make_target(3, 6, None, np.float64, 8) if mode == "target" else None
    mean = a.relax(c, tgt, sl0=1, n=3, first=1, ntr=1)
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new, mean2 = RM.relax(exp[..., 0], c, tgt)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    assert np.array_equal(RM.bits(mean[..., 0]), RM.bits(mean2))
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(RM.bits(ea[k]), RM.bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(RM.bits(e), RM.bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(RM.bits(e[1:4, 3:11, :, 1]), RM.bits(new[:, 3:11]))          # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(RM.bits(ea[k]), RM.bits(eb[k])), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.relax) and callable(mpdata.Plan.relax) and callable(mpdata.Plan.relax_host)
    for nm in ("relax", "relax_shapes"):
        assert nm in mpdata.__all__, nm
    assert mpdata.relax_shapes(5, 3, 8) == {"c": (7, 5), "target": (7, 5), "mean": (7, 5)}
    assert mpdata.relax_shapes(5, 3, 8, 2) == {"c": (7, 5), "target": (2, 7, 5), "mean": (2, 7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3r." in hdr
    sec = hdr.split("---- 3r.")[1].split("---- 4.")[0]
    for word in ("c", "target", "mean", "nx"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels only" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec
    assert hdr.index("---- 3q.") < hdr.index("---- 3r.") < hdr.index("---- 4.")


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
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_relax_device")] == \
        ["plan", "sl0", "n", "c", "target", "mean", "first_tracer", "ntracers"]


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_relax_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_relax_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_relax_device")
    cargs = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert fargs == cargs, (fargs, cargs)
    decl = {}
    for line in m.group(2).splitlines():
        d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\))\s*,\s*value\s*::\s*(.*)", line)
        if d:
            for a in d.group(2).split(","):
                decl[a.strip()] = d.group(1)
    for p, a in zip(params, cargs):
        want = "type(c_ptr)" if "*" in p else "integer(c_int64_t)" if p.startswith("int64_t ") else "integer(c_int)"
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert re.search(r"public ::.*\bmpdata_plan_relax_device_c\b", f90)
    assert "MPDATA_C_PLAN_RELAX" not in f90 and "MPDATA_C_RELAX" not in f90              # no per-precision macro
    # in the second interface block, behind 3p's binding
    assert f90.index("mpdata_plan_cell_add_device_c(plan") < f90.index("mpdata_plan_relax_device_c(plan")
    assert f90.count("\n  interface\n") == 2 and f90.rindex("\n  interface\n") < f90.index("mpdata_plan_relax_device_c(plan")
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "relax_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_relax_device, L.mpdata_relax_f32_device):
        assert fn(4, 0, 6, 1, 0, 4, one, one, None, None, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, one, one, None, None, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 4, one, one, None, None, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, one, one, None, None, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, one, one, None, None, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, None, one, one, one, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, one, None, one, one, None) == mpdata.EINVAL and b"null c" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, 0, 4, None, None, None, None, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()
        assert fn(4, 5, 1, 1, 0, 4, None, None, None, None, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()
    assert L.mpdata_plan_relax_device(None, 0, 1, one, None, None, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error()
    assert L.mpdata_plan_relax(None, 0, 1, one, None, None) == mpdata.EINVAL
    assert L.mpdata_plan_relax_f32(None, 0, 1, one, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_relax_device(one, sl0, n, one, None, None, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_relax_device(one, 0, 0, None, None, None, 0, 1) == mpdata.EINVAL
    assert b"null c" not in L.mpdata_last_error()                                        # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_relax.hip: no scratch memory, no vector and
    no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS, has no barrier and no
    inline assembly"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_relax.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    # target mode and the two forms of mean mode, each f64 and f32; the reference-layout kernel f64 and f32
    assert len(re.findall(r"Function Name: \S*wm_relax_target_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*wm_relax_mean_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*wm_relax_kept_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_relax_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 8 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_relax.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code
    # the bound of the kept form: the one the header and the GPU tests name
    m = re.search(r"constexpr int KEPT_NX = (\d+);", src)
    assert m and int(m.group(1)) == 32
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read().split("---- 3r.")[1].split("---- 4.")[0]
    assert "nx <= 32" in hdr and "nx > 32" in hdr
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_relax\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_relax", mk)
