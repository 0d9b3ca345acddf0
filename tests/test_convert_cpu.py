"""CPU tests of the first-order conversion between two tracers (include/mpdata_hip.h 3t): the numpy model of
tests/convert_model.py against a scalar triple loop and against what the definition implies -- r = 0 levels, exact
conservation without a yield, the LIMIT bound, the ordered dsum, the merge property of level windows --, the plan model's
rules, and the interface (header, ctypes, Fortran, Python names, the argument checks that need no device, the compiler's
resource report).  No test here needs a GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import convert_model as CV
from oracle import plan_model as PM
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_convert_device", "mpdata_plan_convert", "mpdata_plan_convert_f32", "mpdata_convert_device",
         "mpdata_convert_f32_device")
DTYPES = [np.float64, np.float32]
OPTIONS = list(itertools.product((False, True), repeat=3))      # (q0, y, LIMIT)


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    f = rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, T)).astype(dtype)
    f[:, 4, ::3] = -0.0
    return np.asfortranarray(f)


def args(f, src, nz, q0, y, seed):
    n, dt = f.shape[0], f.dtype.type
    return (CV.make_r(n, nz, dt, seed), CV.make_q0(f[..., src]) if q0 else None, CV.make_y(n, nz, dt, seed) if y else None)


# ---- the model against the definition
@pytest.mark.parametrize("q0,y,limit", OPTIONS, ids=["".join(c for c, on in zip("qyL", o) if on) or "none" for o in OPTIONS])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, q0, y, limit):
    n, nx, nz, T = 3, 5, 9, 3
    f = field(n, nx, nz, T, dtype, 11)
    for src, dst in ((0, 2), (2, 0), (1, 0)):
        r, q, yy = args(f, src, nz, q0, y, 12 + src)
        assert (r == 0).any() and (r > 1).any() and ((r > 0) & (r < 1)).any()
        new, dsum = CV.convert(f, src, dst, r, q, yy, limit)
        want, wsum = CV.convert_loops(f, src, dst, r, q, yy, limit)
        assert np.array_equal(bits(new), bits(want)) and np.array_equal(bits(dsum), bits(wsum))
        other = 3 - src - dst
        assert np.array_equal(bits(new[..., other]), bits(f[..., other]))
        assert not np.array_equal(new[..., src], f[..., src]) and not np.array_equal(new[..., dst], f[..., dst])
        changed, off, cap = CV.branch_shares(f, src, dst, r, q, yy, limit)
        assert 0.1 <= changed <= 0.9 and off >= 0.1 and (cap >= 0.1 or not limit), (changed, off, cap)
        if q is not None:                                   # some cells have a == q0 exactly: they take the +0 branch
            assert (f[:, 3:nx + 3, :, src] == q[:, None, :]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_r_zero_levels_keep_every_bit(dtype):
    """... of BOTH tracers, -0.0 included, for r = +0 and r = -0; their dsum is +0.  Computed through, such a level would
    give c + 0 * e, which turns a -0.0 of dst into +0.0"""
    n, nx, nz, T = 3, 4, 9, 3
    f = field(n, nx, nz, T, dtype, 5)
    f[1, 5, 0, 2] = -0.0
    r, q, y = args(f, 0, nz, True, True, 6)
    r[1, 4] = -0.0
    zero = r == 0
    assert zero[1, 4] and zero[1, 0] and not zero.all()
    for limit in (False, True):
        new, dsum = CV.convert(f, 0, 2, r, q, y, limit)
        for b, k in zip(*np.nonzero(zero)):
            assert np.array_equal(bits(new[b, :, k]), bits(f[b, :, k])), (b, k)
            assert dsum[b, k] == 0 and not np.signbit(dsum[b, k])
        assert np.signbit(new[1, 5, 0, 2]) and np.signbit(new[0, 4, 0, 0]) and np.signbit(new[0, 4, 3, 2])
        for b, k in zip(*np.nonzero(~zero & (not limit))):       # (LIMIT: a row with no positive value moves nothing)
            assert not np.array_equal(bits(new[b, 3:nx + 3, k, 0]), bits(f[b, 3:nx + 3, k, 0])), (b, k)
        new0, dsum0 = CV.convert(f, 0, 2, np.zeros_like(r), q, y, limit)
        assert np.array_equal(bits(new0), bits(f)) and not dsum0.any() and not np.signbit(dsum0).any()


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "LIMIT"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_without_a_yield_src_plus_dst_is_conserved_exactly(dtype, limit):
    """small integers and r in {0, 1, 2, 3}: no statement rounds, so src + dst keeps its value in every cell and dsum is the
    amount that left src"""
    n, nx, nz, T = 4, 6, 8, 3
    rng = np.random.default_rng(31)
    f = np.asfortranarray(rng.integers(-8, 9, (n, nx + 6, nz - 1, T)).astype(dtype))
    r = np.asfortranarray(rng.integers(0, 4, (n, nz - 1)).astype(dtype))
    q0 = np.asfortranarray(rng.integers(-2, 3, (n, nz - 1)).astype(dtype))
    new, dsum = CV.convert(f, 1, 0, r, q0, None, limit)
    assert np.array_equal(new[..., 1] + new[..., 0], f[..., 1] + f[..., 0]) and not np.array_equal(new, f)
    assert np.array_equal(dsum, (f[:, 3:nx + 3, :, 1] - new[:, 3:nx + 3, :, 1]).sum(axis=1))
    assert np.array_equal(bits(new[..., 2]), bits(f[..., 2]))


@pytest.mark.parametrize("q0", [False, True], ids=["noq0", "q0"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_limit_never_leaves_src_below_min_a_0(dtype, q0):
    n, nx, nz, T = 3, 7, 11, 3
    f = field(n, nx, nz, T, dtype, 41)
    r, q, y = args(f, 2, nz, q0, True, 42)
    new, _, d, e_raw, capped = CV.convert(f, 2, 0, r, q, y, True, parts=True)
    a = f[:, 3:nx + 3, :, 2]
    assert np.all(new[:, 3:nx + 3, :, 2] >= np.minimum(a, 0)) and capped.any()
    assert np.all(new[:, 3:nx + 3, :, 2][capped & (a > 0)] == 0)            # a - a
    plain = CV.convert(f, 2, 0, r, q, y, False)[0]
    assert (plain[:, 3:nx + 3, :, 2] < np.minimum(a, 0)).any()                # ... which the plain mode does not hold


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_dsum_is_the_ordered_sum_of_the_differences(dtype):
    """s = +0; s = s + d(i) for i = 1 .. nx in the arrays' precision; another order gives other bits somewhere"""
    n, nx, nz, T = 6, 13, 9, 2
    R = dtype
    f = field(n, nx, nz, T, dtype, 51)
    r, q, y = args(f, 0, nz, True, True, 52)
    _, dsum, d, _, _ = CV.convert(f, 0, 1, r, q, y, False, parts=True)
    back = np.zeros_like(dsum)
    for b in range(n):
        for k in range(nz - 1):
            s, t = R(0), R(0)
            for i in range(nx):
                s = R(s + d[b, i, k])
                t = R(t + d[b, nx - 1 - i, k])
            assert bits(np.array(s)) == bits(np.array(dsum[b, k])) or r[b, k] == 0, (b, k)
            back[b, k] = t
    assert np.any(bits(back) != bits(dsum))


@pytest.mark.parametrize("limit", [False, True], ids=["plain", "LIMIT"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 300])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype, limit):
    """the operator on every level window as a problem of its own (r, q0 and y of the tall levels it stands for), owned
    levels merged == the operator on the tall column, bit for bit; dsum from each level's owner.  The geometry is the
    library's."""
    n, nx, T = 2, 3, 3
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    r, q, y = args(f, 2, nz, True, True, 22)
    want, want_s = CV.convert(f, 2, 0, r, q, y, limit)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_s = np.array(f, order="F"), np.full_like(want_s, np.nan)
    got[:, 3:nx + 3, :, 0] = got[:, 3:nx + 3, :, 2] = np.nan
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        sub = lambda x: np.asfortranarray(x[:, lev])
        new, s = CV.convert(np.asfortranarray(f[:, :, lev]), 2, 0, sub(r), sub(q), sub(y), limit)
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, 3:nx + 3, own], got_s[:, own] = new[:, 3:nx + 3, loc], s[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_s), bits(want_s))
    assert not np.array_equal(want, f)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = CV.PlanModelConvert(oracle, *shape, T, dtype)
    return m, CV.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    r = CV.make_r(5, 6, np.float64, 6)
    assert m.convert(0, 2, r) == PM.ESTATE                                      # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.convert(0, 2, r, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for src, dst in ((-1, 0), (0, 3), (3, 0), (1, 1), (0, 0)):
        assert m.convert(src, dst, r) == PM.EINVAL, (src, dst)
    assert m.convert(0, 2, None) == PM.EINVAL and m.convert(0, 2, r, mode=2) == PM.EINVAL and m.convert(0, 2, r, mode=3) == PM.EINVAL
    assert m.convert(0, 2, r, eb=4) == PM.ESTATE                                # a host form of the other precision
    assert m.convert(0, 2, None, eb=4) == PM.EINVAL and m.convert(1, 1, r, eb=4) == PM.EINVAL     # the arguments come first
    m.multi = True
    assert m.convert(0, 2, r) == PM.EUNSUPPORTED and m.convert(0, 2, r, sl0=0, n=0) == PM.EINVAL
    assert m.convert(1, 1, None) == PM.EUNSUPPORTED                             # the handle comes before the pair
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(bits(m.a[k]), bits(v)), k
    dsum = m.convert(0, 2, r)
    assert dsum.shape == (5, 5) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(bits(m.a["f"][:, :3]), bits(keep["f"][:, :3]))        # halo columns keep every bit
    assert np.array_equal(bits(m.a["f"][:, 11:]), bits(keep["f"][:, 11:]))
    assert np.array_equal(bits(m.a["f"][..., 1]), bits(keep["f"][..., 1]))      # ... and so does the third tracer
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(bits(m.a[k]), bits(keep[k])), k


@pytest.mark.parametrize("limit", [0, CV.LIMIT], ids=["plain", "LIMIT"])
@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_convert_is_export_change_import(oracle, boundary, limit):
    """the call on a block = export of the block, the operator, import; on a PERIODIC model the halos of the next
    read-back are wrapped copies of the NEW interior of both tracers"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    r, y = CV.make_r(3, 6, np.float64, 7), CV.make_y(3, 6, np.float64, 7)
    q0 = CV.make_q0(a.a["f"][1:4, ..., 2])
    dsum = a.convert(2, 0, r, q0, y, limit, sl0=1, n=3)
    before = np.array(b.a["f"][1:4], order="F")             # (the model's arrays: export_block would wrap a periodic one)
    new, dsum2 = CV.convert(before, 2, 0, r, q0, y, bool(limit))
    assert b.import_block(1, 3, {"f": new}, 0, 3) is None
    assert np.array_equal(bits(dsum), bits(dsum2))
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(bits(e), bits(PM.wrap(np.array(e, order="F"))))
        for t in (0, 2):
            assert np.array_equal(bits(e[1:4, 3:11, :, t]), bits(new[:, 3:11, :, t]))           # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.convert) and callable(mpdata.Plan.convert) and callable(mpdata.Plan.convert_host)
    for nm in ("convert", "convert_shapes", "CONVERT_LIMIT"):
        assert nm in mpdata.__all__, nm
    assert mpdata.CONVERT_LIMIT == 1 == CV.LIMIT
    assert mpdata.convert_shapes(5, 3, 8) == {"r": (7, 5), "q0": (7, 5), "y": (7, 5), "dsum": (7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3t." in hdr
    sec = hdr.split("---- 3t.")[1].split("---- 4.")[0]
    for word in ("src", "dst", "r", "q0", "y", "dsum", "nx", "MPDATA_CONVERT_LIMIT"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_CONVERT_LIMIT 1\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "rounded once" in sec and "never fmax / fmin" in sec and "mpdata_plan_shard_plan" in sec
    for line in ("e = (e > 0) ? e : +0", "d = r(b,k) * e", "m = (a > 0) ? a : +0 ;  d = (d > m) ? m : d", "f(i,k,src) = a - d",
                 "g = y ? y(b,k) * d : d", "f(i,k,dst) = c + g", "s = +0; do i = 1, nx: s = s + d(i)"):
        assert line in sec, line
    assert hdr.index("---- 3s.") < hdr.index("---- 3t.") < hdr.index("---- 4.")


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
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_convert_device")] == \
        ["plan", "sl0", "n", "src", "dst", "r", "q0", "y", "mode", "dsum"]
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_convert_device")] == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "src", "dst", "r", "q0", "y", "mode", "dsum", "stream"]


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_convert_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_convert_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_convert_device")
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
    assert re.search(r"public ::.*\bmpdata_plan_convert_device_c\b", f90)
    assert re.search(r"MPDATA_CONVERT_LIMIT = 1\b", f90)
    assert "MPDATA_C_PLAN_CONVERT" not in f90 and "MPDATA_C_CONVERT" not in f90            # no per-precision macro
    # in the second interface block, behind 3r's binding
    assert f90.index("mpdata_plan_relax_device_c(plan") < f90.index("mpdata_plan_convert_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "convert_calls.F90"))


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, the pair (outside, then equal), r, the mode"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    for fn in (L.mpdata_convert_device, L.mpdata_convert_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, src=0, dst=2, r=one, mode=0: \
            fn(ncrms, nx, nz, T, sl0, n, f, src, dst, r, None, None, mode, None, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        for src, dst in ((-1, 0), (3, 0), (0, 3), (0, -1)):
            assert call(src=src, dst=dst) == mpdata.EINVAL and b"tracer pair" in err(), (src, dst)
        assert call(src=1, dst=1) == mpdata.EINVAL and b"src == dst" in err()
        assert call(r=None) == mpdata.EINVAL and b"null r" in err()
        for mode in (2, 3, 4, -1):
            assert call(mode=mode) == mpdata.EINVAL and b"mode" in err(), mode
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, src=9, r=None, mode=2) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, src=9, r=None, mode=2) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, src=9, r=None, mode=2) == mpdata.EINVAL and b"null f" in err()
        assert call(src=9, dst=9, r=None, mode=2) == mpdata.EINVAL and b"tracer pair" in err()
        assert call(src=1, dst=1, r=None, mode=2) == mpdata.EINVAL and b"src == dst" in err()
        assert call(r=None, mode=2) == mpdata.EINVAL and b"null r" in err()
    assert L.mpdata_plan_convert_device(None, 0, 1, 0, 1, one, None, None, 0, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_convert(None, 0, 1, 0, 1, one, None, None, 0, None) == mpdata.EINVAL
    assert L.mpdata_plan_convert_f32(None, 0, 1, 0, 1, one, None, None, 0, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_convert_device(one, sl0, n, 0, 1, one, None, None, 0, None) == mpdata.EINVAL
    assert L.mpdata_plan_convert_device(one, 0, 0, 1, 1, None, None, None, 9, None) == mpdata.EINVAL
    assert b"n = 0" in err()                                                             # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_convert.hip: no scratch memory, no vector
    and no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS, has no barrier and
    no inline assembly, and uses compare-and-select, not fmax / fmin"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_convert.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_convert_kernel", txt)) == 2         # double, float2
    assert len(re.findall(r"Function Name: \S*ref_convert_kernel", txt)) == 2        # double, float
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 4 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_convert.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code
    assert not re.search(r"\bf?(max|min)f?\s*\((?!i \+ u)", code)                    # (the one min: the clamped column index)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_convert\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_convert", mk)
    assert "mpdata_convert.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
