"""CPU tests of the per-level covariance of two tracers (include/mpdata_hip.h 3u): the numpy model of
tests/level_cov_model.py against a scalar loop nest and against what the definition implies -- a variance is never
negative, the pair commutes, RAW is the central form about zero, the mean is the relax model's, the distance to a
long-double evaluation stays inside a derived bound, and the variants that are NOT the definition (reversed order, rounded
reciprocal, one-pass formula) differ in bits --, the plan model's rules, and the interface (header, ctypes, Fortran, Python
names, the argument checks that need no device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import level_cov_model as LC
import relax_model as RM
from oracle import plan_model as PM
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_cov_device", "mpdata_plan_level_cov", "mpdata_plan_level_cov_f32", "mpdata_level_cov_device",
         "mpdata_level_cov_f32_device")
DTYPES = [np.float64, np.float32]
PAIRS = ((0, 2), (2, 0), (1, 0), (1, 1))


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    return np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, T)).astype(dtype))


# ---- the model against the definition
@pytest.mark.parametrize("how", list(LC.MEANS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_loop_nest(dtype, how):
    n, nx, nz, T = 3, 5, 9, 3
    f = field(n, nx, nz, T, dtype, 11)
    f[:, :3] = f[:, nx + 3:] = np.nan                       # halo columns are not read
    for ta, tb in PAIRS:
        ma, mb, raw = LC.call_args(n, nz, dtype, 12 + ta, how)
        got = LC.level_cov(f, ta, tb, ma, mb, raw)
        want = LC.level_cov_loops(f, ta, tb, ma, mb, raw)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert g.dtype == dtype and np.array_equal(bits(g), bits(w)) and np.isfinite(g).all()
        if not raw:                                         # the means come back given or formed
            assert ma is None or np.array_equal(bits(got[1]), bits(ma))
            assert mb is None or np.array_equal(bits(got[2]), bits(mb))
        g = np.array(f)
        g[..., [t for t in range(T) if t not in (ta, tb)]] = np.nan      # ... and no other tracer
        assert np.array_equal(bits(LC.level_cov(g, ta, tb, ma, mb, raw)[0]), bits(got[0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_variance_is_never_negative_and_the_pair_commutes(dtype):
    n, nx, nz, T = 5, 7, 28, 3
    f = field(n, nx, nz, T, dtype, 21)
    for how in ("raw", "central", "both"):
        ma, mb, raw = LC.call_args(n, nz, dtype, 22, how)
        for t in range(T):
            v = LC.level_cov(f, t, t, ma, ma, raw)[0]       # (the same profile on both sides)
            assert np.all(v >= 0) and not np.signbit(v).any() and (v > 0).all()
        for ta, tb in ((0, 2), (1, 0)):
            c_ab, m_a, m_b = LC.level_cov(f, ta, tb, ma, mb, raw)
            c_ba, n_b, n_a = LC.level_cov(f, tb, ta, mb, ma, raw)
            assert np.array_equal(bits(c_ab), bits(c_ba))
            assert raw or (np.array_equal(bits(m_a), bits(n_a)) and np.array_equal(bits(m_b), bits(n_b)))
            assert (c_ab < 0).any() and (c_ab > 0).any()    # the covariance of two tracers takes both signs


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_raw_is_the_central_form_about_zero(dtype):
    """x - (+0) keeps every bit of x, so RAW and ma = mb = +0 agree wherever no -0.0 is involved (the field holds none)"""
    n, nx, nz, T = 4, 6, 10, 3
    f = field(n, nx, nz, T, dtype, 31)
    assert not np.signbit(f[f == 0]).any()
    z = np.zeros((n, nz - 1), dtype, order="F")
    for ta, tb in PAIRS:
        raw = LC.level_cov(f, ta, tb, raw=True)
        cen = LC.level_cov(f, ta, tb, z, z)
        assert raw[1] is None and raw[2] is None
        assert np.array_equal(bits(raw[0]), bits(cen[0])) and not cen[1].any() and not cen[2].any()
        assert LC.share_differs(raw[0], LC.level_cov(f, ta, tb)[0]) == 1.0


@pytest.mark.parametrize("nx", [2, 3, 11, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_mean_is_the_relax_models(dtype, nx):
    n, nz, T = 4, 9, 3
    f = field(n, nx, nz, T, dtype, 41)
    one = np.ones((n, nz - 1), dtype, order="F")
    for ta, tb in PAIRS:
        _, m_a, m_b = LC.level_cov(f, ta, tb)
        assert np.array_equal(bits(m_a), bits(RM.relax(np.asfortranarray(f[..., ta]), one)[1]))
        assert np.array_equal(bits(m_b), bits(RM.relax(np.asfortranarray(f[..., tb]), one)[1]))


def bound(f, ta, tb, ma, mb, raw, u):
    """|c_computed - c_exact| per output for arithmetic of unit roundoff u, with g(k) = k u / (1 - k u), A = max |a_i| of
    the row and |m| the exact mean (or the given one):
      formed mean   the nx - 1 rounded adds of s (the first, +0 + a_1, is exact) give |s^ - s| <= g(nx - 1) nx A, the
                    divide one more rounding: e_a = |m^ - m| <= g(nx) A; a given mean and RAW: e_a = 0
      deviation     da^ = (a - m^)(1 + d): |da^ - da| <= ea := e_a (1 + u) + u Da with Da = A + |m| >= |da| (RAW: ea = 0,
                    Da = A)
      product       p^ = da^ db^ (1 + d): |p^ - p| <= ep := Da eb + Db ea + ea eb + u (Da + ea)(Db + eb), and
                    |p^| <= P := (Da + ea)(Db + eb)(1 + u)
      sum           nx - 1 rounded adds: |c^ - sum p^| <= g(nx - 1) nx P
    so |c^ - c| <= nx ep + g(nx - 1) nx P.  One rounding is counted per statement of the definition, none is left out
    and none is estimated from the data."""
    L = np.longdouble
    nx = f.shape[1] - 6
    g = lambda k: L(k) * u / (1 - L(k) * u)
    out = []
    for t, m in ((ta, ma), (tb, mb)):
        x = np.abs(f[:, 3:nx + 3, :, t].astype(L))
        A = x.max(axis=1)
        if raw:
            out.append((A, L(0) * A))
            continue
        formed = m is None
        mm = np.abs(sum(f[:, 3 + i, :, t].astype(L) for i in range(nx)) / L(nx)) if formed else np.abs(np.asarray(m).astype(L))
        e = g(nx) * A if formed else L(0) * A
        D = A + mm
        out.append((D, e * (1 + u) + u * D))
    (Da, ea), (Db, eb) = out
    ep = Da * eb + Db * ea + ea * eb + u * (Da + ea) * (Db + eb)
    P = (Da + ea) * (Db + eb) * (1 + u)
    return nx * ep + g(nx - 1) * nx * P


@pytest.mark.parametrize("how", list(LC.MEANS))
@pytest.mark.parametrize("nx", [2, 3, 17, 33])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_within_the_rounding_bound_of_a_long_double_evaluation(dtype, nx, how):
    """the bound of `bound` for the model's precision plus the same bound for the long-double evaluation itself"""
    L = np.longdouble
    n, nz, T = 4, 9, 3
    f = field(n, nx, nz, T, dtype, 51)
    u, uL = L(np.finfo(dtype).eps) / 2, L(np.finfo(L).eps) / 2
    for ta, tb in PAIRS:
        ma, mb, raw = LC.call_args(n, nz, dtype, 52, how)
        c = LC.level_cov(f, ta, tb, ma, mb, raw)[0]
        ref = LC.long_two_pass(f, ta, tb, ma, mb, raw)
        lim = bound(f, ta, tb, ma, mb, raw, u) + bound(f, ta, tb, ma, mb, raw, uL)
        err = np.abs(c.astype(L) - ref)
        assert np.all(err <= lim), (ta, tb, float(np.max(err / lim)))
        assert np.all(lim <= 8 * nx * (nx + 1) * u)        # (the bound itself is small: |f| < 1/2, so every D < 1)


@pytest.mark.parametrize("nx", [2, 3, 8, 11, 17, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_what_is_not_the_definition_differs_in_bits(dtype, nx):
    """uniform random fields, 5 x nx x 27: the reversed order is the same sum at nx = 2 and another one from nx = 3 on; the
    one-pass formula and RAW are other numbers; the rounded reciprocal is the divide at powers of two and differs at nx =
    3, 11, 17 (in at least one output in fifty)"""
    n, nz, T = 5, 28, 3
    f = field(n, nx, nz, T, dtype, 61)
    tot = {"raw": [], "rev": [], "one": [], "rec": []}
    for ta, tb in PAIRS:
        c = LC.level_cov(f, ta, tb)[0]
        tot["raw"].append(LC.share_differs(c, LC.level_cov(f, ta, tb, raw=True)[0]))
        tot["rev"].append(LC.share_differs(c, LC.level_cov(f, ta, tb, reverse=True)[0]))
        tot["one"].append(LC.share_differs(c, LC.one_pass(f, ta, tb)))
        tot["rec"].append(LC.share_differs(c, LC.level_cov(f, ta, tb, recip=True)[0]))
    s = {k: float(np.mean(v)) for k, v in tot.items()}
    assert s["raw"] >= 0.1 and s["one"] >= 0.1, s
    assert s["rev"] == 0 if nx == 2 else s["rev"] >= 0.1, s
    assert s["rec"] == 0 if nx in (2, 8, 32) else s["rec"] >= 0.02, s


# ---- the plan model: the call changes nothing; the order of the checks
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = LC.PlanModelLevelCov(oracle, *shape, T, dtype)
    return m, LC.make_plan_inputs(oracle, shape, T, dtype, 100)


def _state(m):
    return (m.boundary, m.uploaded, m.have_u, m.have_w, m.timing, m.ran, list(m.steps), list(m.fmax), list(m.flmax))


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_call_changes_no_array_and_no_mark(oracle, boundary):
    m, inp = _model(oracle)
    assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None
    keep, state = {k: np.array(v) for k, v in m.a.items()}, _state(m)
    ma, mb = LC.make_profile(3, 6, np.float64, 1, 0), LC.make_profile(3, 6, np.float64, 1, 1)
    for ta, tb in PAIRS:
        for how, kw in (("raw", dict(mode=LC.RAW)), ("central", dict(mean_a=True, mean_b=True)), ("ma", dict(ma=ma, mean_b=True)),
                        ("both", dict(ma=ma, mb=mb, mean_a=True))):
            c, m_a, m_b = m.level_cov(ta, tb, sl0=1, n=3, **kw)
            want = LC.level_cov(keep["f"][1:4], ta, tb, kw.get("ma"), kw.get("mb"), how == "raw")
            assert np.array_equal(bits(c), bits(want[0])) and c.shape == (3, 5)
            assert (m_a is None) == (not kw.get("mean_a")) and (m_b is None) == (not kw.get("mean_b"))
            assert m_a is None or np.array_equal(bits(m_a), bits(want[1]))
            assert m_b is None or np.array_equal(bits(m_b), bits(want[2]))
            assert _state(m) == state
            for k, v in keep.items():
                assert np.array_equal(bits(m.a[k]), bits(v)), k


def test_plan_model_check_order(oracle):
    m, inp = _model(oracle)
    ma = LC.make_profile(5, 6, np.float64, 2, 0)
    assert m.level_cov(0, 2) == PM.ESTATE                                       # never filled
    assert m.level_cov(0, 3) == PM.EINVAL and m.level_cov(0, 2, cov=False) == PM.EINVAL     # ... the arguments come first
    assert m.upload(inp) is None
    state = _state(m)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.level_cov(0, 2, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for ta, tb in ((-1, 0), (0, 3), (3, 0), (0, -1), (3, 3)):
        assert m.level_cov(ta, tb) == PM.EINVAL, (ta, tb)
    for mode in (2, 3, 4, -2):
        assert m.level_cov(0, 2, mode=mode) == PM.EINVAL, mode
    for kw in (dict(ma=ma), dict(mb=ma), dict(mean_a=True), dict(mean_b=True)):
        assert m.level_cov(0, 2, mode=LC.RAW, **kw) == PM.EINVAL, kw
    assert m.level_cov(0, 2, cov=False) == PM.EINVAL
    assert m.level_cov(0, 2, eb=4) == PM.ESTATE                                 # a host form of the other precision
    assert m.level_cov(0, 2, eb=4, cov=False) == PM.EINVAL and m.level_cov(0, 9, eb=4) == PM.EINVAL
    m.multi = True
    assert m.level_cov(0, 2) == PM.EUNSUPPORTED and m.level_cov(0, 2, sl0=0, n=0) == PM.EINVAL
    assert m.level_cov(9, 9, cov=False) == PM.EUNSUPPORTED                      # the handle comes before the pair
    m.multi = False
    assert _state(m) == state
    assert not isinstance(m.level_cov(1, 1), int)                               # ta == tb is allowed


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.level_cov) and callable(mpdata.Plan.level_cov) and callable(mpdata.Plan.level_cov_host)
    for nm in ("level_cov", "level_cov_shapes", "LEVEL_COV_RAW"):
        assert nm in mpdata.__all__, nm
    assert mpdata.LEVEL_COV_RAW == 1 == LC.RAW
    assert mpdata.level_cov_shapes(5, 3, 8) == {k: (7, 5) for k in ("ma", "mb", "cov", "mean_a", "mean_b")}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3u." in hdr
    sec = hdr.split("---- 3u.")[1].split("---- 4.")[0]
    for word in ("ta", "tb", "ma", "mb", "cov", "mean_a", "mean_b", "nx", "MPDATA_LEVEL_COV_RAW"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_LEVEL_COV_RAW 1\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec and "ta == tb" in sec
    assert "not divided by nx and not by nx - 1" in sec and "rounded reciprocal" in sec
    for line in ("mode & MPDATA_LEVEL_COV_RAW :  da_i = a_i ;  db_i = b_i",
                 "m_a = ma ? ma(b,k) : ( s = +0; do i = 1, nx: s = s + a_i ;  s / nx )",
                 "m_b = mb ? mb(b,k) : the same from b_i",
                 "mean_a(b,k) = m_a ;  mean_b(b,k) = m_b",
                 "da_i = a_i - m_a ;  db_i = b_i - m_b",
                 "c = +0;  do i = 1, nx:  p = da_i * db_i ;  c = c + p",
                 "cov(b,k) = c"):
        assert line in sec, line
    assert hdr.index("---- 3t.") < hdr.index("---- 3u.") < hdr.index("---- 4.")


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
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_level_cov_device")] == \
        ["plan", "sl0", "n", "ta", "tb", "ma", "mb", "mode", "cov", "mean_a", "mean_b"]
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_level_cov_device")] == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "ta", "tb", "ma", "mb", "mode", "cov", "mean_a", "mean_b", "stream"]
    assert _c_params(hdr, "mpdata_level_cov_device")[6].startswith("const ")        # f is only read


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_level_cov_device_c\(([^)]*)\)\s*&?\s*"
                  r"bind\(C, name=\"mpdata_plan_level_cov_device\"\)(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_level_cov_device")
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
    assert re.search(r"public ::.*\bmpdata_plan_level_cov_device_c\b", f90)
    assert re.search(r"MPDATA_LEVEL_COV_RAW = 1\b", f90)
    assert "MPDATA_C_PLAN_LEVEL_COV" not in f90 and "MPDATA_C_LEVEL_COV" not in f90        # no per-precision macro
    # in the second interface block, behind 3t's binding
    assert f90.index("mpdata_plan_convert_device_c(plan") < f90.index("mpdata_plan_level_cov_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert f90.rindex("\n  interface\n") < f90.index("mpdata_plan_level_cov_device_c(plan")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "level_cov_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\blevel_cov\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, the pair, the mode bits, RAW with a
    profile or a mean output, cov"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    for fn in (L.mpdata_level_cov_device, L.mpdata_level_cov_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, ta=0, tb=2, ma=None, mb=None, mode=0, cov=one, mean_a=None, \
            mean_b=None: fn(ncrms, nx, nz, T, sl0, n, f, ta, tb, ma, mb, mode, cov, mean_a, mean_b, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        for ta, tb in ((-1, 0), (3, 0), (0, 3), (0, -1), (3, 3)):
            assert call(ta=ta, tb=tb) == mpdata.EINVAL and b"tracer pair" in err(), (ta, tb)
        for mode in (2, 3, 4, -1):
            assert call(mode=mode) == mpdata.EINVAL and b"mode bits" in err(), mode
        for k in ("ma", "mb", "mean_a", "mean_b"):
            assert call(mode=1, **{k: one}) == mpdata.EINVAL and b"MPDATA_LEVEL_COV_RAW with a non-null " + k.encode() in err(), k
        assert call(cov=None) == mpdata.EINVAL and b"null cov" in err()
        assert call(mode=1, cov=None) == mpdata.EINVAL and b"null cov" in err()
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, ta=9, mode=3, ma=one, cov=None) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, ta=9, mode=3, ma=one, cov=None) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, ta=9, mode=3, ma=one, cov=None) == mpdata.EINVAL and b"null f" in err()
        assert call(ta=9, mode=3, ma=one, cov=None) == mpdata.EINVAL and b"tracer pair" in err()
        assert call(mode=3, ma=one, cov=None) == mpdata.EINVAL and b"mode bits" in err()
        assert call(mode=1, ma=one, cov=None) == mpdata.EINVAL and b"non-null ma" in err()
    dev = lambda plan=one, sl0=0, n=1, ta=0, tb=1, ma=None, mode=0, cov=one: \
        L.mpdata_plan_level_cov_device(plan, sl0, n, ta, tb, ma, None, mode, cov, None, None)
    assert dev(plan=None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_cov(None, 0, 1, 0, 1, None, None, 0, one, None, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_cov_f32(None, 0, 1, 0, 1, None, None, 0, one, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert dev(sl0=sl0, n=n) == mpdata.EINVAL
    assert dev(n=0, ta=9, mode=9, cov=None) == mpdata.EINVAL and b"n = 0" in err()     # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_level_cov.hip: no scratch memory, no vector
    and no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS, has no barrier and
    no inline assembly.  Kernels: the plan-layout one in its three forms (one-pass, re-read, kept), each for one stream
    (ta == tb) and two, each for double and float2 elements; the reference-layout one for double and float."""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_level_cov.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_level_cov_kernel", txt)) == 12
    assert len(re.findall(r"Function Name: \S*ref_level_cov_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 14 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_level_cov.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_level_cov\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_level_cov", mk)
    assert "mpdata_level_cov$(O)" in mk.split("OBJS :=")[1].split("\n")[0]
    assert "mpdata_level_cov.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
