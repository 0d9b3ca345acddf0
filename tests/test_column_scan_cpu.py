"""CPU tests of the running column integrals (include/mpdata_hip.h 3aa): the numpy model of tests/column_scan_model.py
against a scalar triple loop and against what the definition implies -- the total that is 3k's path, the reversed sum, the
shift between the inclusive and the exclusive result, the carry across level windows --, the plan model's rules, and the
interface (header, ctypes, Fortran, Python names, the argument checks that need no device, the compiler's resource
report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import column_path_model as CP
import column_scan_model as CS
from oracle import plan_model as PM
from util import assert_bitwise, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_column_scan_device", "mpdata_plan_column_scan", "mpdata_plan_column_scan_f32", "mpdata_column_scan_device",
         "mpdata_column_scan_f32_device")
DTYPES = [np.float64, np.float32]
MODE_IDS = ["up", "down", "up-excl", "down-excl"]
T = 3
PAIRS = ((0, 2), (2, 0), (1, 1))      # (src, dst): dst above, below and equal to src


def field(n, nx, nz, ntr, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, ntr])
    return np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, ntr)).astype(dtype))


def rho_adz(n, nz, dtype, seed):
    rng = np.random.default_rng([seed, n, nz, 5])
    return tuple(np.asfortranarray(rng.uniform(0.5, 1.0, (n, nz - 1)).astype(dtype)) for _ in range(2))


# ---- the model against the definition
@pytest.mark.parametrize("mode", CS.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, mode):
    n, nx, nz = 3, 5, 9
    f = field(n, nx, nz, T, dtype, 11)
    f[1, 4, 2::3] = -0.0
    for q, (src, dst) in enumerate(PAIRS):
        w = CS.make_wgt(n, nz, dtype, 12 + q)
        new, tot = CS.column_scan(f, src, dst, w, mode)
        want, wt = CS.column_scan_loops(f, src, dst, w, mode)
        assert_bitwise(new, want, f"f, src {src} dst {dst}")
        assert_bitwise(tot, wt, f"total, src {src} dst {dst}")
        for t in range(T):
            if t != dst:
                assert_bitwise(new[..., t], f[..., t], f"tracer {t}")
        assert_bitwise(new[:, :3], f[:, :3], "halos") or assert_bitwise(new[:, nx + 3:], f[:, nx + 3:], "halos")
        assert not np.array_equal(bits(new[..., dst]), bits(f[..., dst]))
        inner = new[:, 3:nx + 3, :, dst]
        assert not np.signbit(inner[inner == 0]).any()                 # s starts at +0.0: no -0.0 comes out
        if mode & CS.EXCLUSIVE:
            first = inner[:, :, -1 if mode & CS.DOWN else 0]
            assert np.all(first == 0) and not np.signbit(first).any()  # the first o of an EXCLUSIVE scan is +0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_product_is_rounded_before_the_add(dtype):
    """an fma (the product exact, one rounding per level) gives other bits somewhere: the inputs tell the two apart"""
    n, nx, nz = 4, 9, 30
    f = field(n, nx, nz, T, dtype, 13)
    w = CS.make_wgt(n, nz, dtype, 14)
    new, _ = CS.column_scan(f, 0, 1, w)
    s = np.zeros((n, nx), np.longdouble)
    fused = np.empty((n, nx, nz - 1), dtype)
    for k in range(nz - 1):
        s = (s + w[:, None, k].astype(np.longdouble) * f[:, 3:nx + 3, k, 0].astype(np.longdouble)).astype(dtype).astype(np.longdouble)
        fused[:, :, k] = s
    assert not np.array_equal(bits(new[:, 3:nx + 3, :, 1]), bits(fused))
    assert np.allclose(new[:, 3:nx + 3, :, 1], fused, rtol=1e-3 if dtype == np.float32 else 1e-10, atol=1e-5)


@pytest.mark.parametrize("excl", [0, CS.EXCLUSIVE], ids=["incl", "excl"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_up_total_with_rho_adz_is_the_path_of_3k(dtype, excl):
    n, nx, nz = 4, 7, 28
    f = field(n, nx, nz, T, dtype, 15)
    rho, adz = rho_adz(n, nz, dtype, 16)
    path = CP.column_path(f, rho, adz)[0]                              # (n, nx, T)
    for src in range(T):
        new, tot = CS.column_scan(f, src, (src + 1) % T, CS.weights(rho, adz), excl)
        assert_bitwise(tot, path[:, :, src], f"total of tracer {src}")
        if not excl:
            assert_bitwise(new[:, 3:nx + 3, nz - 2, (src + 1) % T], path[:, :, src], "level nzm of the inclusive UP scan")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_down_total_is_the_reversed_sum(dtype):
    n, nx, nz = 4, 7, 28
    f = field(n, nx, nz, T, dtype, 17)
    rho, adz = rho_adz(n, nz, dtype, 18)
    rev = CP.path_reversed(f, rho, adz)
    up = CP.column_path(f, rho, adz)[0]
    assert not np.array_equal(bits(rev), bits(up))                     # the order of the levels shows in the bits
    for excl in (0, CS.EXCLUSIVE):
        _, tot = CS.column_scan(f, 1, 1, CS.weights(rho, adz), CS.DOWN | excl)
        assert_bitwise(tot, rev[:, :, 1], "DOWN total")


@pytest.mark.parametrize("down", [0, CS.DOWN], ids=["up", "down"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_exclusive_is_inclusive_shifted_by_one_level(dtype, down):
    """an identity on o, not arithmetic: o_excl at a level is o_incl at the level walked just before it, the first o_excl is
    +0.0, and the last o_incl is total of both.  (o_incl - o_excl reproduces p only where that subtraction is exact.)"""
    n, nx, nz = 3, 6, 19
    f = field(n, nx, nz, T, dtype, 19)
    w = CS.make_wgt(n, nz, dtype, 20)
    inc, ti = CS.column_scan(f, 0, 2, w, down)
    exc, te = CS.column_scan(f, 0, 2, w, down | CS.EXCLUSIVE)
    oi, oe = inc[:, 3:nx + 3, :, 2], exc[:, 3:nx + 3, :, 2]
    if down:
        oi, oe = oi[:, :, ::-1], oe[:, :, ::-1]                        # in the order of the walk
    assert_bitwise(np.ascontiguousarray(oe[:, :, 1:]), np.ascontiguousarray(oi[:, :, :-1]), "the shift")
    assert_bitwise(np.ascontiguousarray(oe[:, :, 0]), np.zeros((n, nx), dtype), "the first o")
    assert_bitwise(ti, te, "total") or assert_bitwise(np.ascontiguousarray(oi[:, :, -1]), ti, "the last inclusive o")


@pytest.mark.parametrize("mode", CS.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 300])
def test_windows_with_the_carry_merge_to_the_tall_scan(mpdata, nz, dtype, mode):
    """a tall column scanned window by window over the OWNED levels, UP through the windows upward and DOWN downward, s
    carried from window to window, wgt addressed by the tall level == the tall scan, bit for bit.  The geometry is the
    library's.  Without the carry, or with wgt addressed by the window's level, the bits differ."""
    n, nx = 2, 3
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 21)
    w = CS.make_wgt(n, nz, dtype, 22)
    want, want_t = CS.column_scan(f, 0, 1, w, mode)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    x = np.array(f[:, 3:nx + 3, :, 0])
    got = np.array(f, order="F")
    got[:, 3:nx + 3, :, 1] = np.nan
    nocarry, local = np.array(got), np.array(got)
    s = np.zeros((n, nx), dtype)
    owned = np.zeros(nzm, int)
    for h in (range(W - 1, -1, -1) if mode & CS.DOWN else range(W)):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = list(range(own0 - 1, own1))                              # tall, 0-based
        if mode & CS.DOWN:
            lev = lev[::-1]
        o, s_new = CS.scan_carried(x, w, s, lev, bool(mode & CS.EXCLUSIVE))
        o0, _ = CS.scan_carried(x, w, np.zeros((n, nx), dtype), lev, bool(mode & CS.EXCLUSIVE))
        wl = np.zeros_like(w)
        wl[:, lev] = w[:, [k - k0 for k in lev]]                       # the mutant: the window's level
        ol, _ = CS.scan_carried(x, wl, s, lev, bool(mode & CS.EXCLUSIVE))
        for k in lev:
            got[:, 3:nx + 3, k, 1], nocarry[:, 3:nx + 3, k, 1], local[:, 3:nx + 3, k, 1] = o[k], o0[k], ol[k]
            owned[k] += 1
        s = s_new
    assert np.all(owned == 1)
    assert_bitwise(got, want, "f") or assert_bitwise(s, want_t, "total")
    assert not np.array_equal(bits(nocarry), bits(want)) and not np.array_equal(bits(local), bits(want))


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, ntr=T, shape=(5, 8, 6)):
    m = CS.PlanModelColumnScan(oracle, *shape, ntr, dtype)
    return m, CS.make_plan_inputs(oracle, shape, ntr, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    assert m.column_scan(0, 1) == PM.ESTATE                                      # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.column_scan(0, 1, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for t in (-1, T):
        assert m.column_scan(t, 0) == PM.EINVAL and m.column_scan(0, t) == PM.EINVAL
    for mode in (4, 5, 8, -1):
        assert m.column_scan(0, 1, mode=mode) == PM.EINVAL, mode
    assert m.column_scan(0, 1, eb=4) == PM.ESTATE                                # a host form of the other precision
    assert m.column_scan(T, 1, eb=4) == PM.EINVAL and m.column_scan(0, 1, mode=4, eb=4) == PM.EINVAL   # the arguments come first
    m.multi = True
    assert m.column_scan(0, 1) == PM.EUNSUPPORTED and m.column_scan(0, 1, sl0=0, n=0) == PM.EINVAL
    assert m.column_scan(9, 9, mode=4) == PM.EUNSUPPORTED                        # the handle comes before src, dst and the mode
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(bits(m.a[k]), bits(v)), k
    tot = m.column_scan(1, 0)
    assert tot.shape == (5, 8) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(bits(m.a["f"][:, :3]), bits(keep["f"][:, :3]))         # halo columns keep every bit
    assert np.array_equal(bits(m.a["f"][:, 11:]), bits(keep["f"][:, 11:]))
    assert np.array_equal(bits(m.a["f"][..., 1:]), bits(keep["f"][..., 1:]))     # ... and so do the other tracers, src among them
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(bits(m.a[k]), bits(keep[k])), k
    assert_bitwise(tot, CP.column_path(keep["f"], keep["rho"], keep["adz"])[0][:, :, 1], "wgt None: the path of 3k")


@pytest.mark.parametrize("mode", CS.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_column_scan_is_export_change_import(oracle, boundary, mode):
    """the call on a block = export of the block, the scan, import of dst; on a PERIODIC model the halos of the next
    read-back are wrapped copies of the NEW interior of dst, and those of src are what they were.  The block (1, 3) of five
    instances splits the pairs an fp32 plan would form at both ends: the neighbours 0 and 4 keep every bit, a planted -0.0
    among them."""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
        m.a["f"][0, 4, ::2, 2] = -0.0
        m.a["f"][4, 4, ::2, 2] = -0.0
    w = CS.make_wgt(3, 6, np.float64, 7)
    tot = a.column_scan(0, 2, w, mode, sl0=1, n=3)
    before = np.array(b.a["f"], order="F")                  # (the model's arrays: export_block would wrap a periodic one)
    new, t2 = CS.column_scan(before[1:4], 0, 2, w, mode)
    assert b.import_block(1, 3, {"f": np.asfortranarray(new[..., 2])}, 2, 1) is None
    assert np.array_equal(bits(tot), bits(t2))
    for sl in (0, 4):
        assert np.array_equal(bits(a.a["f"][sl]), bits(before[sl])) and np.signbit(a.a["f"][sl, 4, ::2, 2]).all()
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(bits(e), bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(bits(e[1:4, 3:11, :, 2]), bits(new[:, 3:11, :, 2]))               # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k


def test_plan_model_last_instance_of_an_odd_plan(oracle):
    """a block that holds instance ncrms - 1 of an odd plan (the phantom's partner) and one that misses it: the model changes
    the block alone"""
    m, inp = _model(oracle)
    assert m.upload(inp) is None
    keep = np.array(m.a["f"])
    assert not isinstance(m.column_scan(2, 2, None, CS.DOWN, sl0=4, n=1), int)
    assert np.array_equal(bits(m.a["f"][:4]), bits(keep[:4])) and not np.array_equal(m.a["f"][4], keep[4])
    keep = np.array(m.a["f"])
    assert not isinstance(m.column_scan(2, 0, None, 0, sl0=3, n=1), int)
    assert np.array_equal(bits(m.a["f"][4]), bits(keep[4])) and np.array_equal(bits(m.a["f"][:3]), bits(keep[:3]))


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.column_scan) and callable(mpdata.Plan.column_scan) and callable(mpdata.Plan.column_scan_host)
    for nm in ("column_scan", "column_scan_shapes", "COLUMN_SCAN_DOWN", "COLUMN_SCAN_EXCLUSIVE"):
        assert nm in mpdata.__all__, nm
    assert mpdata.COLUMN_SCAN_DOWN == 1 == CS.DOWN and mpdata.COLUMN_SCAN_EXCLUSIVE == 2 == CS.EXCLUSIVE
    assert mpdata.column_scan_shapes(5, 3, 8) == {"wgt": (7, 5), "total": (3, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3aa." in hdr
    sec = hdr.split("---- 3aa.")[1].split("---- 4.")[0]
    for word in ("src", "dst", "wgt", "total", "mode", "nx", "MPDATA_COLUMN_SCAN_DOWN", "MPDATA_COLUMN_SCAN_EXCLUSIVE"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_COLUMN_SCAN_DOWN 1\b", sec) and re.search(r"#define MPDATA_COLUMN_SCAN_EXCLUSIVE 2\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "one rounded operation" in sec and "no contraction" in sec and "mpdata_plan_shard_plan" in sec
    assert "the reference tree has no such routine" in sec
    for line in ("p(k) = wgt(b,k) * f(sl,i,k,src)", "UP (default):  s = +0.0;  k = 1 .. nzm", "DOWN:          s = +0.0;  k = nzm .. 1",
                 "inclusive (default):  s = s + p(k);  o(k) = s", "EXCLUSIVE:            o(k) = s;      s = s + p(k)",
                 "f(sl,i,k,dst) = o(k);     total(b,i) = the final s"):
        assert line in sec, line
    for rule in ("dst's halos keep\n *     every bit", "no wrap is launched in front; only the halo mark of dst is cleared afterwards",
                 "The mark of src is not touched.", "only the seam mark of dst is cleared",
                 "the phantom half follows instance ncrms - 1 in dst", "stores the partner's half of dst back as loaded",
                 "The first o of an EXCLUSIVE scan is +0.0", "read once and written once"):
        assert rule in sec, rule
    assert hdr.index("---- 3z.") < hdr.index("---- 3aa.") < hdr.index("---- 4.")


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
    tail = ["src", "dst", "wgt", "total", "mode"]
    for n in NAMES[:3]:
        assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)] == ["plan", "sl0", "n"] + tail
    for n in NAMES[3:]:
        assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)] == ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f"] + tail + ["stream"]


def test_fortran_interface_agrees_with_the_header():
    """the five interfaces, bound by their literal names, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    for name in NAMES:
        m = re.search(r"integer\(c_int\) function " + name + r"_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"" + name + r"\"\)(.*?)end function", f90, re.S)
        assert m, name
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        params = _c_params(hdr, name)
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
            assert decl.get(a) == want, (name, a, p, decl.get(a))
        assert re.search(r"public ::.*\b" + name + r"_c\b", f90), name
    assert re.search(r"MPDATA_COLUMN_SCAN_DOWN = 1\b", f90) and re.search(r"MPDATA_COLUMN_SCAN_EXCLUSIVE = 2\b", f90)
    assert f90.index("mpdata_combine_f32_device_c(ncrms") < f90.index("mpdata_plan_column_scan_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "column_scan_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\bcolumn_scan\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, wgt, src, dst, the mode"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    for fn in (L.mpdata_column_scan_device, L.mpdata_column_scan_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, ntr=3, sl0=0, n=4, f=one, src=0, dst=1, wgt=one, mode=0: \
            fn(ncrms, nx, nz, ntr, sl0, n, f, src, dst, wgt, None, mode, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(ntr=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        assert call(wgt=None) == mpdata.EINVAL and b"null wgt" in err()
        for t in (-1, 3):
            assert call(src=t) == mpdata.EINVAL and b"src" in err(), t
            assert call(dst=t) == mpdata.EINVAL and b"dst" in err(), t
        for mode in (4, 5, 8, -1):
            assert call(mode=mode) == mpdata.EINVAL and b"mode" in err(), mode
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, wgt=None, src=9, dst=9, mode=4) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, wgt=None, src=9, dst=9, mode=4) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, wgt=None, src=9, dst=9, mode=4) == mpdata.EINVAL and b"null f" in err()
        assert call(wgt=None, src=9, dst=9, mode=4) == mpdata.EINVAL and b"null wgt" in err()
        assert call(src=9, dst=9, mode=4) == mpdata.EINVAL and b"src" in err()
        assert call(dst=9, mode=4) == mpdata.EINVAL and b"dst" in err()
    for fn in (L.mpdata_plan_column_scan_device, L.mpdata_plan_column_scan, L.mpdata_plan_column_scan_f32):
        assert fn(None, 0, 1, 0, 1, None, None, 0) == mpdata.EINVAL and b"null plan" in err()
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_column_scan_device(one, sl0, n, 0, 1, None, None, 0) == mpdata.EINVAL
    assert L.mpdata_plan_column_scan_device(one, 0, 0, 9, 9, None, None, 9) == mpdata.EINVAL
    assert b"n = 0" in err()                                                             # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_column_scan.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel, at most 128 allocated VGPRs (four waves per SIMD, what 40 KiB of LDS a
    workgroup leave room for); the LDS of the plan-layout kernel is dynamic, its budget the constant mpdata_vsolve.hip and
    the other staging kernels keep; direction and inclusion are no template arguments: one staging code per element type
    and kind of plan"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_column_scan.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_column_scan_kernel", txt)) == 4      # double, float2; plain, windowed
    assert len(re.findall(r"Function Name: \S*ref_column_scan_kernel", txt)) == 2     # double, float
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 6 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", txt)]
    assert len(vgprs) == 6 and max(vgprs) <= 128, vgprs
    src = open(os.path.join(csrc, "mpdata_column_scan.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "LDS_ELEMS" in code and "col_groups_batched" in code
    assert not re.search(r"__shfl|__reduce|dpp|ds_swizzle|readlane", code)           # no reduction or scan across lanes
    assert not re.search(r"\bfma\w*\s*\(", code)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_column_scan\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_column_scan", mk)
    assert re.search(r"mpdata_plan_blocks\$\(O\):.*mpdata_column_scan\.h", mk)
    assert "mpdata_column_scan.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
