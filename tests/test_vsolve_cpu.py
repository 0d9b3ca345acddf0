"""CPU tests of the implicit vertical solve (include/mpdata_hip.h 3o): the numpy model of tests/vsolve_model.py against
what is not itself -- exact integer cases where A x == f must hold to the bit, the dense fp64 solve of numpy.linalg on
the random class --, the sweep cut at the owned ranges of the library's level windows with the carries handed over, the
plan model's rules, and the interface (header, ctypes, Fortran, Python names, the argument checks that need no device,
the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import vsolve_model as VM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_vsolve_device", "mpdata_plan_vsolve", "mpdata_plan_vsolve_f32", "mpdata_vsolve_device",
         "mpdata_vsolve_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


def apply_matrix(x, lo, di, up):
    """A x on the interior columns, in float64 (exact for the small integers of the exact cases)"""
    n, nxp6, nzm = x.shape[:3]
    X = x.reshape(x.shape[:3] + (-1,)).astype(np.float64)
    out = di[:, None, :, None].astype(np.float64) * X
    out[:, :, 1:] += lo[:, None, 1:, None].astype(np.float64) * X[:, :, :-1]
    out[:, :, :-1] += up[:, None, :-1, None].astype(np.float64) * X[:, :, 1:]
    return out.reshape(x.shape)


# ---- 1. the model against something that is not itself
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("side", ["lower", "upper"])
def test_exact_bidiagonal_integer_cases(dtype, side):
    """di = 1, one of lo, up zero, the other integers in [-2, 2], f integers in [-3, 3], nzm <= 12: every intermediate is a
    small integer (|x| <= 3 * (3^12 - 1) / 2 < 2^24), so A x == f holds exactly in both precisions"""
    worst = 0.0
    for seed in range(12):
        rng = np.random.default_rng([31, seed])
        n, nx, nzm, T = 3, 2, int(rng.integers(2, 13)), 2
        f = np.asfortranarray(rng.integers(-3, 4, (n, nx + 6, nzm, T)).astype(dtype))
        off = np.asfortranarray(rng.integers(-2, 3, (n, nzm)).astype(dtype))
        zero, one = np.zeros((n, nzm), dtype, order="F"), np.ones((n, nzm), dtype, order="F")
        lo, up = (off, zero) if side == "lower" else (zero, off)
        x = VM.vsolve(f, lo, one, up)
        assert x.dtype == np.dtype(dtype)
        assert np.array_equal(apply_matrix(x, lo, one, up)[:, 3:nx + 3], f[:, 3:nx + 3].astype(np.float64))
        assert np.array_equal(VM.bits(x[:, :3]), VM.bits(f[:, :3])) and np.array_equal(VM.bits(x[:, nx + 3:]), VM.bits(f[:, nx + 3:]))
        worst = max(worst, float(np.max(np.abs(x))))
    assert worst > 3                                         # the off-diagonal did something


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_identity_and_one_level(dtype):
    """lo = up = 0, di = 1 keeps every bit on inputs without -0.0, and the stated exception; nzm = 1: x = f * (1 / di)"""
    n, nx, nz = 3, 4, 9
    f = field(n, nx, nz, 2, dtype, 5)
    f[0, 4, 2] = 0.0
    assert not np.any(np.signbit(f) & (f == 0))
    zero, one = np.zeros((n, nz - 1), dtype, order="F"), np.ones((n, nz - 1), dtype, order="F")
    assert np.array_equal(VM.bits(VM.vsolve(f, zero, one, zero)), VM.bits(f))
    # the exception: f = -0.0 above a negative y: m = 0 * y = -0.0, r = -0.0 - -0.0 = +0.0
    z = np.zeros((1, 7, 2), dtype, order="F")
    z[0, 3, 0], z[0, 3, 1] = -1.0, -0.0
    x = VM.vsolve(z, zero[:1, :2], one[:1, :2], zero[:1, :2])
    assert x[0, 3, 0] == -1.0 and x[0, 3, 1] == 0 and not np.signbit(x[0, 3, 1])
    # one level: lo and up are not read at all
    f1 = field(n, nx, 2, 1, dtype, 6)
    di = np.asfortranarray(np.random.default_rng(7).uniform(1.0, 2.0, (n, 1)).astype(dtype))
    nan = np.full((n, 1), np.nan, dtype, order="F")
    x = VM.vsolve(f1, nan, di, nan)
    R = np.dtype(dtype).type
    want = np.array(f1)
    want[:, 3:nx + 3] = f1[:, 3:nx + 3] * (R(1) / di)[:, None, :]
    assert np.array_equal(VM.bits(x), VM.bits(want))


def test_ends_of_lo_and_up_are_not_read():
    n, nx, nz = 2, 3, 7
    f = field(n, nx, nz, 1, np.float64, 8)
    lo, di, up = VM.make_coeffs(n, nz, np.float64, 9)
    want = VM.vsolve(f, lo, di, up)
    lo2, up2 = np.array(lo, order="F"), np.array(up, order="F")
    lo2[:, 0], up2[:, -1] = np.nan, np.nan
    assert np.array_equal(VM.bits(VM.vsolve(f, lo2, di, up2)), VM.bits(want))


RANDOM_NZM = (1, 2, 27, 64, 237, 999)
RANDOM_SEEDS = 20
# measured with the seeds below, in units of u * max|f| (u = half the spacing at 1): the worst over RANDOM_NZM and the seeds
MEASURED = {np.float64: 3.01, np.float32: 2.64}
BOUND = {k: 4 * v for k, v in MEASURED.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_random_class_against_the_dense_fp64_solve(dtype):
    """the random class (lo, up in [-0.4, 0), di = 1 - lo - up: the inverse has infinity norm <= 1) against
    numpy.linalg.solve on float64 copies of the same inputs, in units of u * max|f|.  The yardstick is the dense fp64
    solve, not the code under test.  Measured over nzm = 1, 2, 27, 64, 237, 999 and 20 seeds: worst 3.009 (fp64) and 2.633
    (fp32); the bound is 4 x that, 12.04 and 10.56 -- the factor is the margin for other seeds.  max|x| / max|f| stays
    below 1 (0.9846 at most with these seeds)."""
    u = float(np.finfo(dtype).eps) / 2
    worst, growth = 0.0, 0.0
    for nzm in RANDOM_NZM:
        for seed in range(RANDOM_SEEDS):
            n, nx = 2, 2
            f = field(n, nx, nzm + 1, 1, dtype, 40 + seed)
            lo, di, up = VM.make_coeffs(n, nzm + 1, dtype, 60 + seed)
            x = VM.vsolve(f, lo, di, up)
            fmax = float(np.max(np.abs(f[:, 3:nx + 3])))
            for b in range(n):
                A = np.diag(di[b].astype(np.float64)) + np.diag(lo[b, 1:].astype(np.float64), -1) + np.diag(up[b, :-1].astype(np.float64), 1)
                ref = np.linalg.solve(A, f[b, 3:nx + 3].astype(np.float64).T).T
                worst = max(worst, float(np.max(np.abs(x[b, 3:nx + 3].astype(np.float64) - ref))) / (u * fmax))
            growth = max(growth, float(np.max(np.abs(x[:, 3:nx + 3]))) / fmax)
    print(f"vsolve against the dense fp64 solve, {np.dtype(dtype).name}: worst {worst:.3f} u max|f| (bound {BOUND[dtype]}), "
          f"max|x| / max|f| {growth:.4f}")
    assert worst <= BOUND[dtype]
    assert growth <= 1.0


# ---- 2. windows: the sweep cut at the owned ranges with the carries handed over == the tall solve, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 250, 300, 1000])
def test_windows_with_carries_are_the_tall_solve(mpdata, nz, dtype):
    """a numpy restatement of the windowed kernel's order: the windows upward, each continuing the forward sweep on its
    OWNED levels with y(k-1) of the window below and the coefficients of the tall levels it stands for, y stored; then
    downward, each continuing the backward sweep with x(k+1) of the window above.  The geometry is the library's."""
    n, nx, T = 2, 3, 2
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    lo, di, up = VM.make_coeffs(n, nz, dtype, 22)
    want = VM.vsolve(f, lo, di, up)
    p, g = VM.factor(lo, di, up)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    own = []
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        assert k0 + 1 <= own0 <= own1 <= k0 + nz_w - 1
        own.append(slice(own0 - 1, own1))                    # tall, 0-based
    assert own[0].start == 0 and own[-1].stop == nzm and all(a.stop == b.start for a, b in zip(own, own[1:]))
    got = np.array(f, order="F")
    c = got[:, 3:nx + 3]                                     # (a view: the sweeps store into got)
    carry = None
    for s in own:                                            # upward
        c[:, :, s], carry = VM.forward(np.array(c[:, :, s]), lo[:, s], p[:, s], carry, s.start)
    carry = None
    for s in reversed(own):                                  # downward: what the upward walk stored
        c[:, :, s], carry = VM.backward(np.array(c[:, :, s]), g[:, s], carry)
    assert np.array_equal(VM.bits(got), VM.bits(want))
    assert not np.array_equal(want, f)


# ---- 3. the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = VM.PlanModelVsolve(oracle, *shape, T, dtype)
    return m, VM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    c = VM.make_coeffs(5, 6, np.float64, 6)
    assert m.vsolve(*c) == PM.ESTATE                                       # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.vsolve(*c, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.vsolve(*c, first=1, ntr=2) == PM.EINVAL and m.vsolve(*c, first=-1, ntr=1) == PM.EINVAL
    assert m.vsolve(*c, first=0, ntr=0) == PM.EINVAL
    for i in range(3):
        a = list(c)
        a[i] = None
        assert m.vsolve(*a) == PM.EINVAL
        assert m.vsolve(*a, eb=4) == PM.EINVAL                             # the NULL comes before the precision
    assert m.vsolve(*c, eb=4) == PM.ESTATE                                 # a host form of the other precision
    m.multi = True
    assert m.vsolve(*c) == PM.EUNSUPPORTED and m.vsolve(*c, sl0=0, n=0) == PM.EINVAL
    assert m.vsolve(None, None, None) == PM.EUNSUPPORTED                   # the handle comes before the NULL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(VM.bits(m.a[k]), VM.bits(v)), k
    assert m.vsolve(*c) is None and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(VM.bits(m.a["f"][:, :3]), VM.bits(keep["f"][:, :3]))            # halo columns keep every bit
    assert np.array_equal(VM.bits(m.a["f"][:, 11:]), VM.bits(keep["f"][:, 11:]))
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(VM.bits(m.a[k]), VM.bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_vsolve_is_export_change_import(oracle, boundary):
    """the call on a block and a tracer = export of the block, the solve, import; on a PERIODIC model the halos of the
    next read-back are wrapped copies of the NEW interior"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    c = VM.make_coeffs(3, 6, np.float64, 7)
    assert a.vsolve(*c, sl0=1, n=3, first=1, ntr=1) is None
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new = VM.vsolve(exp[..., 0], *c)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(VM.bits(ea[k]), VM.bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(VM.bits(e), VM.bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(VM.bits(e[1:4, 3:11, :, 1]), VM.bits(new[:, 3:11]))          # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(VM.bits(ea[k]), VM.bits(eb[k])), k


# ---- 4. the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.vsolve) and callable(mpdata.Plan.vsolve) and callable(mpdata.Plan.vsolve_host)
    assert "vsolve" in mpdata.__all__ and "vsolve_shapes" in mpdata.__all__
    assert mpdata.vsolve_shapes(5, 8) == {"lo": (7, 5), "di": (7, 5), "up": (7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    sec = hdr.split("---- 3o.")[1].split("---- 4.")[0]
    for word in ("lo", "di", "up", "pivoting"):
        assert re.search(r"\b" + word + r"\b", sec, re.I), word
    assert "windowed plans" in sec.lower() and "are supported" in sec and "-0.0" in sec
    assert "second read and write" in sec


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
    m = re.search(r"integer\(c_int\) function mpdata_plan_vsolve_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_vsolve_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_vsolve_device")
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
    assert re.search(r"public ::.*\bmpdata_plan_vsolve_device_c\b", f90)
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "vsolve_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_vsolve_device, L.mpdata_vsolve_f32_device):
        assert fn(4, 0, 6, 1, 0, 4, one, one, one, one, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, one, one, one, one, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 4, one, one, one, one, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, one, one, one, one, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, one, one, one, one, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
        for i, nm in enumerate(("f", "lo", "di", "up")):
            args = [one, one, one, one]
            args[i] = None
            assert fn(4, 5, 6, 1, 0, 4, *args, None) == mpdata.EINVAL, nm
            assert b"null " + nm.encode() in L.mpdata_last_error()
        assert fn(4, 5, 1, 1, 0, 4, None, None, None, None, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()      # sizes first
        assert fn(4, 5, 6, 1, 2, 3, None, None, None, None, None) == mpdata.EINVAL and b"outside" in L.mpdata_last_error()   # then the block
        assert fn(4, 5, 6, 1, 0, 4, None, None, one, None, None) == mpdata.EINVAL and b"null f" in L.mpdata_last_error()     # then f
        assert fn(4, 5, 6, 1, 0, 4, one, None, one, None, None) == mpdata.EINVAL and b"null lo" in L.mpdata_last_error()     # then lo, di, up
    assert L.mpdata_plan_vsolve_device(None, 0, 1, one, one, one, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error()
    assert L.mpdata_plan_vsolve(None, 0, 1, one, one, one) == mpdata.EINVAL
    assert L.mpdata_plan_vsolve_f32(None, 0, 1, one, one, one) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_vsolve_device(one, sl0, n, one, one, one, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_vsolve_device(one, 0, 0, None, None, None, 0, 1) == mpdata.EINVAL
    assert b"null lo" not in L.mpdata_last_error()                                  # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_vsolve.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel; the LDS of the plan-layout kernel is dynamic, its budget a constant of
    the file: 40 KiB at most, four workgroups per CU"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_vsolve.usage.txt")
    assert os.path.exists(rep), "no resource-usage report: the library is built by __graft_entry__.build()"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_vsolve_kernel", txt)) == 4       # f64 and f32, plain and windowed
    assert len(re.findall(r"Function Name: \S*vsolve_factor_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_vsolve_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 8 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_vsolve.hip")).read()
    walk = open(os.path.join(csrc, "mpdata_wm_walk.h")).read()
    m = re.search(r"constexpr int LDS_ELEMS = (\d+);", walk)                               # (the one statement of the limit)
    assert m and int(m.group(1)) * 8 <= 40 * 1024
    assert "col_groups_batched(j, b.sel, wg, LDS_ELEMS," in src and "g->lds_e <= budget" in walk     # the launch refuses more
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule = re.search(r"mpdata_vsolve\$\(O\):.*\n\t(.*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(1) and "CC_USAGE" in rule.group(1)
