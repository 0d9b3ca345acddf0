"""CPU tests of the linear combinations of tracers (include/mpdata_hip.h 3z): the numpy model of tests/combine_model.py
against a scalar triple loop and against what the definition implies -- the bit copy, the degenerate form that is 3i's
level_add, the sum that is 3g's, the merge property of level windows --, the plan model's rules, and the interface (header,
ctypes, Fortran, Python names, the argument checks that need no device, the compiler's resource report).  No test here
needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import combine_model as CB
import level_add_model as AM
import level_stats_model as LM
from oracle import plan_model as PM
from util import assert_bitwise, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_combine_device", "mpdata_plan_combine", "mpdata_plan_combine_f32", "mpdata_combine_device",
         "mpdata_combine_f32_device")
DTYPES = [np.float64, np.float32]
T = 9
# nsrc -> (dst, src): dst above, below and among the sources, repeated sources, eight distinct sources and a ninth dst
LISTS = {0: [(2, ())], 1: [(0, (3,)), (3, (3,)), (5, (1,))], 2: [(1, (0, 2)), (2, (2, 2)), (0, (4, 0))],
         3: [(8, (0, 4, 2)), (4, (0, 4, 0)), (0, (5, 3, 1))], 8: [(8, (0, 1, 2, 3, 4, 5, 6, 7)), (3, (7, 3, 0, 3, 8, 1, 3, 2))]}
OPTIONS = [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, True, True), (False, False, True)]


def field(n, nx, nz, ntr, dtype, seed, specials=False):
    rng = np.random.default_rng([seed, n, nx, nz, ntr])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, ntr)).astype(dtype))
    return CB.plant_specials(f)[0] if specials else f


# ---- the model against the definition
@pytest.mark.parametrize("coef,c0,clip", OPTIONS, ids=["".join(c for c, on in zip("acL", o) if on) or "none" for o in OPTIONS])
@pytest.mark.parametrize("nsrc", list(LISTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, nsrc, coef, c0, clip):
    n, nx, nz = 3, 5, 9
    f = field(n, nx, nz, T, dtype, 11, specials=True)
    assert np.isnan(f).any() and np.isinf(f).any() and np.signbit(f[f == 0]).any()
    for q, (dst, src) in enumerate(LISTS[nsrc]):
        a, c = CB.call_args(n, nz, nsrc, dtype, 12 + q, coef, c0)
        new, s = CB.combine(f, dst, src, a, c, clip)
        want, ws = CB.combine_loops(f, dst, src, a, c, clip)
        CB.same(new, want, f"f, dst {dst} src {src}")
        CB.same(s, ws, f"sum, dst {dst} src {src}")
        for t in range(T):
            if t != dst:
                assert_bitwise(new[..., t], f[..., t], f"tracer {t}")
        assert_bitwise(new[:, :3], f[:, :3], "halos") or assert_bitwise(new[:, nx + 3:], f[:, nx + 3:], "halos")
        if nsrc > 1 or coef or c0 or clip or src != (dst,):
            assert not np.array_equal(bits(new[..., dst]), bits(f[..., dst]))
        if clip:
            inner = new[:, 3:nx + 3, :, dst]
            assert not np.isnan(inner).any() and (inner >= 0).all() and not np.signbit(inner[inner == 0]).any()
            assert 0.1 <= np.mean(inner == 0) <= 0.95 or nsrc == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_order_of_the_sources_matters(dtype):
    """another association of the adds, or c0 first, gives other bits somewhere: the inputs tell the orders apart"""
    n, nx, nz = 4, 9, 12
    f = field(n, nx, nz, T, dtype, 13)
    src = (0, 1, 2, 3)
    a, c = CB.call_args(n, nz, 4, dtype, 14, True, True)
    new = CB.combine(f, 8, src, a, c)[0]
    rev = CB.combine(f, 8, src[::-1], np.asfortranarray(a[..., ::-1]), c)[0]
    assert not np.array_equal(bits(new), bits(rev))
    x = [f[:, 3:nx + 3, :, t] for t in src]
    c_first = ((((c[:, None] + a[:, None, :, 0] * x[0]) + a[:, None, :, 1] * x[1]) + a[:, None, :, 2] * x[2]) + a[:, None, :, 3] * x[3])
    assert c_first.dtype == dtype and not np.array_equal(bits(new[:, 3:nx + 3, :, 8]), bits(c_first))
    fused = np.zeros((n, nx, nz - 1), np.longdouble)           # every product exact, rounded once at the end of each add
    for j in range(4):
        fused = (fused + a[:, None, :, j].astype(np.longdouble) * x[j].astype(np.longdouble)).astype(dtype).astype(np.longdouble)
    fused = (fused + c[:, None]).astype(dtype)
    assert not np.array_equal(bits(new[:, 3:nx + 3, :, 8]), bits(fused))         # ... and so does an fma


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_one_source_alone_is_a_copy_of_bits(dtype):
    """nsrc = 1, no coef, no c0: NaN payloads of both signs, infinities and -0.0 arrive as they are"""
    n, nx, nz = 3, 4, 18
    f, mask = CB.plant_specials(field(n, nx, nz, T, dtype, 5))
    src = f[:, 3:nx + 3, :, 3]
    assert len(np.unique(bits(src[np.isnan(src)]))) > 4 and np.signbit(src[np.isnan(src)]).any() and not np.signbit(src[np.isnan(src)]).all()
    assert np.isinf(src).any() and np.signbit(src[src == 0]).any()
    new, s = CB.combine(f, 6, (3,))
    assert_bitwise(new[:, 3:nx + 3, :, 6], src, "the copy")
    assert_bitwise(new[:, :3, :, 6], f[:, :3, :, 6], "halos of dst") or assert_bitwise(new[:, nx + 3:, :, 6], f[:, nx + 3:, :, 6], "halos of dst")
    same, _ = CB.combine(f, 3, (3,))
    assert_bitwise(same, f, "onto itself")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_the_degenerate_form_is_level_add(dtype):
    """nsrc = 1, src = [dst], c0 = d, no coef: the bits of 3i's ADD on the interior columns"""
    n, nx, nz = 4, 6, 11
    f = field(n, nx, nz, 3, dtype, 7)
    f[:, 4, ::3] = -0.0
    d = CB.make_c0(n, nz, dtype, 8)
    new, _ = CB.combine(f, 1, (1,), None, d)
    want = AM.level_add(np.asfortranarray(f[..., 1]), d)
    assert_bitwise(new[:, 3:nx + 3, :, 1], want[:, 3:nx + 3], "interior")
    assert_bitwise(new[:, :3, :, 1], f[:, :3, :, 1], "level_add moves the halos too, combine does not")
    assert not np.array_equal(want[:, :3], f[:, :3, :, 1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_sum_is_the_level_sum_of_the_new_row(dtype):
    n, nx, nz = 5, 13, 9
    f = field(n, nx, nz, T, dtype, 9)
    a, c = CB.call_args(n, nz, 3, dtype, 10, True, True)
    for clip in (False, True):
        new, s = CB.combine(f, 2, (2, 5, 7), a, c, clip)
        assert_bitwise(s, LM.level_stats(np.asfortranarray(new[..., 2]))[0], f"clip {clip}")
        assert not np.array_equal(bits(s), bits(LM.sum_reversed(np.asfortranarray(new[..., 2]))))


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "CLIP"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 300])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype, clip):
    """the operator on every level window as a problem of its own (coef and c0 of the tall levels it stands for), owned
    levels merged == the operator on the tall column, bit for bit; sum from each level's owner.  The geometry is the
    library's."""
    n, nx, ntr = 2, 3, 4
    nzm = nz - 1
    f = field(n, nx, nz, ntr, dtype, 21)
    src = (2, 0, 3)
    a, c = CB.call_args(n, nz, 3, dtype, 22, True, True)
    want, want_s = CB.combine(f, 0, src, a, c, clip)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, got_s = np.array(f, order="F"), np.full_like(want_s, np.nan)
    got[:, 3:nx + 3, :, 0] = np.nan
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, s = CB.combine(np.asfortranarray(f[:, :, lev]), 0, src, np.asfortranarray(a[:, lev]), np.asfortranarray(c[:, lev]), clip)
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, 3:nx + 3, own, 0], got_s[:, own] = new[:, 3:nx + 3, loc, 0], s[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)
    assert_bitwise(got, want, "f") or assert_bitwise(got_s, want_s, "sum")
    assert not np.array_equal(want, f)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, ntr=4, shape=(5, 8, 6)):
    m = CB.PlanModelCombine(oracle, *shape, ntr, dtype)
    return m, CB.make_plan_inputs(oracle, shape, ntr, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    c0 = CB.make_c0(5, 6, np.float64, 6)
    assert m.combine(0, (1, 2)) == PM.ESTATE                                    # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.combine(0, (1, 2), sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for dst in (-1, 4):
        assert m.combine(dst, (1,)) == PM.EINVAL
    assert m.combine(0, (1,) * 9) == PM.EINVAL and m.combine(0, 2) == PM.EINVAL                 # too many; a null src
    for src in ((-1,), (0, 4), (1, 2, 3, 9)):
        assert m.combine(0, src) == PM.EINVAL, src
    assert m.combine(0, ()) == PM.EINVAL and m.combine(0, None) == PM.EINVAL                    # no source, no c0
    assert m.combine(0, (1,), mode=2) == PM.EINVAL and m.combine(0, (1,), mode=3) == PM.EINVAL
    assert m.combine(0, (1,), eb=4) == PM.ESTATE                                # a host form of the other precision
    assert m.combine(0, (), eb=4) == PM.EINVAL and m.combine(4, (1,), eb=4) == PM.EINVAL        # the arguments come first
    m.multi = True
    assert m.combine(0, (1,)) == PM.EUNSUPPORTED and m.combine(0, (1,), sl0=0, n=0) == PM.EINVAL
    assert m.combine(9, (9,)) == PM.EUNSUPPORTED                                # the handle comes before dst
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(bits(m.a[k]), bits(v)), k
    s = m.combine(0, (1, 2), None, c0)
    assert s.shape == (5, 5) and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(bits(m.a["f"][:, :3]), bits(keep["f"][:, :3]))        # halo columns keep every bit
    assert np.array_equal(bits(m.a["f"][:, 11:]), bits(keep["f"][:, 11:]))
    assert np.array_equal(bits(m.a["f"][..., 1:]), bits(keep["f"][..., 1:]))    # ... and so do the other tracers
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(bits(m.a[k]), bits(keep[k])), k


@pytest.mark.parametrize("clip", [0, CB.CLIP], ids=["plain", "CLIP"])
@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_combine_is_export_change_import(oracle, boundary, clip):
    """the call on a block = export of the block, the operator, import of dst; on a PERIODIC model the halos of the next
    read-back are wrapped copies of the NEW interior of dst"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    coef, c0 = CB.call_args(3, 6, 3, np.float64, 7, True, True)
    s = a.combine(2, (0, 2, 3), coef, c0, clip, sl0=1, n=3)
    before = np.array(b.a["f"][1:4], order="F")             # (the model's arrays: export_block would wrap a periodic one)
    new, s2 = CB.combine(before, 2, (0, 2, 3), coef, c0, bool(clip))
    assert b.import_block(1, 3, {"f": np.asfortranarray(new[..., 2])}, 2, 1) is None
    assert np.array_equal(bits(s), bits(s2))
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


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.combine) and callable(mpdata.Plan.combine) and callable(mpdata.Plan.combine_host)
    for nm in ("combine", "combine_shapes", "COMBINE_CLIP", "COMBINE_MAX"):
        assert nm in mpdata.__all__, nm
    assert mpdata.COMBINE_CLIP == 1 == CB.CLIP and mpdata.COMBINE_MAX == 8 == CB.MAX
    assert mpdata.combine_shapes(5, 3, 8, 4) == {"coef": (4, 7, 5), "c0": (7, 5), "sum": (7, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3z." in hdr
    sec = hdr.split("---- 3z.")[1].split("---- 4.")[0]
    for word in ("src", "dst", "nsrc", "coef", "c0", "sum", "nx", "MPDATA_COMBINE_CLIP", "MPDATA_COMBINE_MAX"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_COMBINE_CLIP 1\b", sec) and re.search(r"#define MPDATA_COMBINE_MAX 8\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "rounded once" in sec and "never fmax / fmin" in sec and "mpdata_plan_shard_plan" in sec
    assert "the reference tree has no such routine" in sec
    for line in ("nsrc >= 1:  v = coef ? coef(b,k,0) * x_0 : x_0",
                 "do j = 1, nsrc-1:  p = coef ? coef(b,k,j) * x_j : x_j ;  v = v + p",
                 "c0 given:  v = v + c0(b,k)",
                 "nsrc == 0:  v = c0(b,k)                                (c0 required)",
                 "mode & MPDATA_COMBINE_CLIP:  v = (v > 0) ? v : +0      (so NaN and -0 give +0)",
                 "f(i,k,dst) = v",
                 "sum(b,k):  s = +0; do i = 1, nx: s = s + v(i)          (NULL: skipped; the sum of 3g of the NEW dst row)"):
        assert line in sec, line
    for rule in ("GIVEN plans: halos keep every bit.", "no wrap\n *     is launched; the halo mark of dst is cleared afterwards",
                 "The sources' marks are not touched.", "clears the seam mark\n *     of dst afterwards",
                 "the phantom half follows instance ncrms - 1 in dst", "stores the partner back as loaded"):
        assert rule in sec, rule
    assert hdr.index("---- 3y.") < hdr.index("---- 3z.") < hdr.index("---- 4.")


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
    tail = ["dst", "nsrc", "src", "coef", "c0", "mode", "sum"]
    for n in NAMES[:3]:
        assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)] == ["plan", "sl0", "n"] + tail
    for n in NAMES[3:]:
        assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)] == ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f"] + tail + ["stream"]
    assert all("const int* src" in ", ".join(_c_params(hdr, n)) for n in NAMES)


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
    assert re.search(r"MPDATA_COMBINE_CLIP = 1\b", f90) and re.search(r"MPDATA_COMBINE_MAX = 8\b", f90)
    assert "MPDATA_C_PLAN_COMBINE" not in f90 and "MPDATA_C_COMBINE" not in f90            # no per-precision macro
    # in the second interface block, behind 3y's bindings
    assert f90.index("mpdata_satadj_f32_device_c(ncrms") < f90.index("mpdata_plan_combine_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "combine_calls.F90"))


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, dst, nsrc, a null src, the sources, a null
    c0 without a source, the mode"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    ints = lambda *t: ctypes.cast((ctypes.c_int * len(t))(*t), ctypes.c_void_p)
    s12, bad, many = ints(1, 2), ints(1, 4), ints(*([1] * 9))
    for fn in (L.mpdata_combine_device, L.mpdata_combine_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, ntr=4, sl0=0, n=4, f=one, dst=0, nsrc=2, src=s12, c0=None, mode=0: \
            fn(ncrms, nx, nz, ntr, sl0, n, f, dst, nsrc, src, None, c0, mode, None, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(ntr=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        for dst in (-1, 4):
            assert call(dst=dst) == mpdata.EINVAL and b"dst" in err(), dst
        for nsrc, src in ((-1, s12), (9, many)):
            assert call(nsrc=nsrc, src=src) == mpdata.EINVAL and b"nsrc" in err(), nsrc
        assert call(src=None) == mpdata.EINVAL and b"null src" in err()
        assert call(src=bad) == mpdata.EINVAL and b"src[1]" in err()
        assert call(src=ints(-1, 0)) == mpdata.EINVAL and b"src[0]" in err()
        assert call(nsrc=0, src=None) == mpdata.EINVAL and b"null c0" in err()
        for mode in (2, 3, 4, -1):
            assert call(mode=mode) == mpdata.EINVAL and b"mode" in err(), mode
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, dst=9, nsrc=9, src=None, mode=2) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, dst=9, nsrc=9, src=None, mode=2) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, dst=9, nsrc=9, src=None, mode=2) == mpdata.EINVAL and b"null f" in err()
        assert call(dst=9, nsrc=9, src=None, mode=2) == mpdata.EINVAL and b"dst" in err()
        assert call(nsrc=9, src=None, mode=2) == mpdata.EINVAL and b"nsrc" in err()
        assert call(src=None, mode=2) == mpdata.EINVAL and b"null src" in err()
        assert call(src=bad, mode=2) == mpdata.EINVAL and b"src[1]" in err()
        assert call(nsrc=0, src=None, mode=2) == mpdata.EINVAL and b"null c0" in err()
        assert call(nsrc=0, src=None, c0=one, mode=2) == mpdata.EINVAL and b"mode" in err()
    for fn in (L.mpdata_plan_combine_device, L.mpdata_plan_combine, L.mpdata_plan_combine_f32):
        assert fn(None, 0, 1, 0, 2, s12, None, None, 0, None) == mpdata.EINVAL and b"null plan" in err()
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_combine_device(one, sl0, n, 0, 2, s12, None, None, 0, None) == mpdata.EINVAL
    assert L.mpdata_plan_combine_device(one, 0, 0, 9, 9, None, None, None, 9, None) == mpdata.EINVAL
    assert b"n = 0" in err()                                                             # the range came first


def test_new_kernels_fit_128_registers_without_spill_or_lds():
    """the resource-usage report the build writes next to the object of mpdata_combine.hip: no scratch memory, no vector and
    no scalar register spilled, no static LDS and at most 128 allocated VGPRs (four waves per SIMD) in every kernel; the
    file asks for no dynamic LDS, has no barrier and no inline assembly, and uses compare-and-select, not fmax / fmin"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_combine.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_combine_kernel", txt)) == 18        # nsrc 0 .. 8 of double, float2
    assert len(re.findall(r"Function Name: \S*ref_combine_kernel", txt)) == 18       # nsrc 0 .. 8 of double, float
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 36 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", txt)]
    assert len(vgprs) == 36 and max(vgprs) <= 128, vgprs
    src = open(os.path.join(csrc, "mpdata_combine.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code
    assert not re.search(r"\bf?(max|min)f?\s*\((?!i \+ u)", code)                    # (the one min: the clamped column index)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_combine\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_combine", mk)
    assert re.search(r"mpdata_plan_blocks\$\(O\):.*mpdata_combine\.h", mk)
    assert "mpdata_combine.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
