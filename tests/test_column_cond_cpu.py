"""CPU tests of the per-column conditional level counts, tops and paths (include/mpdata_hip.h 3w): the numpy model of
tests/column_cond_model.py against a plain-Python triple loop and against what the definition implies -- with every level
in, cpath and mass are 3k's path and mass bit for bit; the counts of 3v summed over the levels are the counts of 3w summed
over the columns; an excluded infinity or NaN reaches no cpath --, the guard that every variant that is NOT the definition
changes an output at every shape the GPU tests run, the plan model's rules, and the interface (header, ctypes, Fortran,
Python names, the argument checks that need no device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import column_cond_model as CC
import column_path_model as CP
import level_cond_model as LC
from oracle import plan_model as PM
from test_plan_column_cond import KINDS, SEEDS, TRIPLES
from test_plan_column_cond_sequences import CASES
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_column_cond_device", "mpdata_plan_column_cond", "mpdata_plan_column_cond_f32", "mpdata_column_cond_device",
         "mpdata_column_cond_f32_device")
DTYPES = [np.float64, np.float32]


def arrays(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, T)).astype(dtype))
    rho = np.asfortranarray(rng.uniform(0.5, 1.5, (n, nz - 1)).astype(dtype))
    adz = np.asfortranarray(rng.uniform(0.5, 1.5, (n, nz - 1)).astype(dtype))
    return f, rho, adz


def same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)))


# ---- the model against the definition
@pytest.mark.parametrize("bounds", CC.BOUNDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_plain_triple_loop(dtype, bounds):
    n, nx, nz, T = 3, 5, 11, 3
    f, rho, adz = arrays(n, nx, nz, T, dtype, 11)
    f[:, :3] = f[:, nx + 3:] = np.nan                       # halo columns are not read
    for tc, first, ntr in TRIPLES + ((0, 0, 0),):
        lo, hi = CC.call_args(f, tc, bounds, 12 + tc)
        got = CC.column_cond(f, rho, adz, tc, lo, hi, first, ntr)
        want = CC.column_cond_loops(f, rho, adz, tc, lo, hi, first, ntr)
        for k in CC.OUTPUTS:
            assert same(got[k], want[k]), k
            assert got[k] is None or (got[k].dtype == dtype and np.isfinite(got[k]).all()), k
        assert got["kcnt"].shape == got["kbot"].shape == got["ktop"].shape == (n, nx) and got["cover"].shape == (n,)
        assert ntr == 0 or (got["cpath"].shape == (n, nx, ntr) and got["mass"].shape == (n, ntr))
        g = np.array(f)
        g[..., [t for t in range(T) if t != tc and not first <= t < first + ntr]] = np.nan      # ... and no other tracer
        assert same(CC.column_cond(g, rho, adz, tc, lo, hi, first, ntr)["cpath"], got["cpath"])
        # what the outputs imply of each other
        q, bot, top = got["kcnt"], got["kbot"], got["ktop"]
        assert ((q == 0) == (bot == 0)).all() and ((q == 0) == (top == 0)).all()
        assert (top[q > 0] - bot[q > 0] + 1 >= q[q > 0]).all() and (bot <= top).all() and (top <= nz - 1).all()
        assert np.array_equal(got["cover"], (q > 0).sum(axis=1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_band_of_levels_through_an_infinite_lo_and_empty_levels(dtype):
    """lo = +inf shuts a level out in every column, and so does lo >= hi: a call restricted to levels 3 .. 6 counts, finds
    and sums those alone"""
    n, nx, nz, T = 3, 4, 10, 2
    f, rho, adz = arrays(n, nx, nz, T, dtype, 21)
    hi = np.full((n, nz - 1), np.inf, dtype, order="F")
    lo = np.full((n, nz - 1), np.inf, dtype, order="F")
    lo[:, 2:6] = -np.inf
    r = CC.column_cond(f, rho, adz, 0, lo, hi, 0, T)
    assert (r["kcnt"] == 4).all() and (r["kbot"] == 3).all() and (r["ktop"] == 6).all() and (r["cover"] == nx).all()
    band = np.array(f)
    band[:, :, :2] = band[:, :, 6:] = 0
    assert same(r["cpath"], CP.column_path(band, rho, adz)[0])
    z = CC.column_cond(f, rho, adz, 0, hi, hi, 0, T)        # lo >= hi everywhere
    for k in CC.OUTPUTS:
        assert not z[k].any() and not np.signbit(z[k]).any(), k


# ---- the two identities
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_every_level_in_gives_the_bits_of_column_path(oracle, dtype):
    inp = CC.make_plan_inputs(oracle, (5, 7, 28), 3, dtype, 100)
    lo, hi = CC.all_in(inp["f"], 1)
    for first, ntr in ((0, 3), (1, 2), (2, 1)):
        r = CC.column_cond(inp["f"], inp["rho"], inp["adz"], 1, lo, hi, first, ntr)
        path, mass = CP.column_path(inp["f"][..., first:first + ntr], inp["rho"], inp["adz"])
        assert same(r["cpath"], path) and same(r["mass"], mass)
        assert (r["kcnt"] == 27).all() and (r["kbot"] == 1).all() and (r["ktop"] == 27).all() and (r["cover"] == 7).all()


@pytest.mark.parametrize("bounds", CC.BOUNDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_counts_of_level_cond_and_column_cond_have_the_same_sum(oracle, dtype, bounds):
    inp = CC.make_plan_inputs(oracle, (5, 7, 28), 3, dtype, 100)
    for tc in range(3):
        lo, hi = CC.call_args(inp["f"], tc, bounds, 30 + tc)
        cnt = LC.level_cond(inp["f"], tc, lo, hi, 0, 0)[0]
        kcnt = CC.column_cond(inp["f"], inp["rho"], inp["adz"], tc, lo, hi, 0, 0)["kcnt"]
        a, b = cnt.astype(np.float64).sum(axis=1), kcnt.astype(np.float64).sum(axis=1)
        assert np.array_equal(a, b) and a.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_excluded_infinities_and_nans_reach_no_path_but_a_multiplied_mask_lets_them_in(dtype):
    n, nx, nz, T = 5, 7, 12, 3
    f, rho, adz = arrays(n, nx, nz, T, dtype, 41)
    for tc, t, bounds in ((0, 2, "both"), (2, 1, "lo"), (1, 0, "hi")):
        lo, hi = CC.call_args(f, tc, bounds, 42)
        P = CC.plant(f, tc, lo, hi, t)
        assert np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        r, clean = CC.column_cond(P, rho, adz, tc, lo, hi, 0, T), CC.column_cond(f, rho, adz, tc, lo, hi, 0, T)
        assert np.isfinite(r["cpath"]).all() and np.isfinite(r["mass"]).all()
        for k in CC.OUTPUTS:
            assert same(r[k], clean[k]), k                  # ... as if nothing had been planted
        bad = CC.column_cond(P, rho, adz, tc, lo, hi, t, 1, multiply=True)["cpath"][..., 0]
        q = r["kcnt"]
        assert np.isnan(bad[q < nz - 1]).all() and np.isfinite(bad[q == nz - 1]).all() and (q < nz - 1).any()
    # on a finite field the multiplied mask is the definition, bit for bit: only a planted field tells it apart
    lo, hi = CC.call_args(f, 0, "both", 43)
    assert same(CC.column_cond(f, rho, adz, 0, lo, hi, 0, T, multiply=True)["cpath"], CC.column_cond(f, rho, adz, 0, lo, hi, 0, T)["cpath"])


def test_local_level_of_a_windowed_column(mpdata):
    """the model's window geometry is the library's (mpdata.level_window needs no device), every level has one owner, and the
    window-local index differs from the tall one above the first window"""
    for nz in (239, 250, 300):
        W = CC.level_window(nz, 0)[0]
        assert W > 1
        owned = np.zeros(nz - 1, int)
        for h in range(W):
            got = mpdata.level_window(nz, h)                  # (W, k0, nz_w, own0, own1)
            _, k0, own0, own1 = CC.level_window(nz, h)
            assert (got[0], got[1], got[3], got[4]) == (W, k0, own0, own1), (nz, h, got)
            owned[own0 - 1:own1] += 1
        assert (owned == 1).all()
        loc = CC.local_level(nz)
        _, _, _, own1 = CC.level_window(nz, 0)
        assert np.array_equal(loc[:own1], np.arange(1, own1 + 1)) and (loc[own1:] < np.arange(own1 + 1, nz)).all() and (loc >= 1).all()


# ---- the shapes of the GPU tests: the drawn inputs tell the variants apart
SHAPES = sorted({(k[0], np.dtype(k[2]).name, bool(k[3].get("tall")), SEEDS[name]) for name, k in KINDS.items()})


@pytest.mark.parametrize("shape,dtn,tall,seed", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{d}" for s, d, _, _ in SHAPES])
def test_drawn_inputs_tell_the_variants_apart(oracle, shape, dtn, tall, seed):
    """on the arrays the GPU tests upload, over their four triples with both bounds: every variant of the model that is not
    the definition changes at least one element of at least one output (windowed shapes: the window-local level index
    too)"""
    inp = CC.make_plan_inputs(oracle, shape, 3, np.dtype(dtn).type, seed)
    d = CC.variants_that_change(inp, TRIPLES, nz_windowed=shape[2] if tall else None)
    assert all(d.values()), d


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_sequence_inputs_tell_the_variants_apart(oracle, case):
    name, shape, T, dt, sw, seed = case
    inp = LC.make_plan_inputs(oracle, shape, T, dt, 100 + seed)
    d = CC.variants_that_change(inp, TRIPLES, nz_windowed=shape[2] if sw.get("tall") else None)
    assert all(d.values()), d


# ---- the plan model: the call changes nothing; the order of the checks
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = CC.PlanModelColumnCond(oracle, *shape, T, dtype)
    return m, CC.make_plan_inputs(oracle, shape, T, dtype, 100)


def _state(m):
    return (m.boundary, m.uploaded, m.have_u, m.have_w, m.timing, m.ran, list(m.steps), list(m.fmax), list(m.flmax))


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_call_changes_no_array_and_no_mark(oracle, boundary):
    m, inp = _model(oracle)
    assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None
    keep, state = {k: np.array(v) for k, v in m.a.items()}, _state(m)
    b = slice(1, 4)
    for tc, first, ntr in TRIPLES:
        for bounds in CC.BOUNDS:
            lo, hi = CC.call_args(keep["f"][b], tc, bounds, 5)
            for outs in (CC.OUTPUTS, ("kcnt", "cover"), ("ktop", "kbot"), ("cpath",), ("cpath", "mass")):
                got = m.column_cond(tc, lo, hi, first, ntr, sl0=1, n=3, outs=outs)
                want = CC.column_cond(keep["f"][b], keep["rho"][b], keep["adz"][b], tc, lo, hi, first, ntr if "cpath" in outs else 0)
                assert tuple(got) == tuple(outs)
                for k in outs:
                    assert same(got[k], want[k]), k
                assert _state(m) == state
                for k, v in keep.items():
                    assert np.array_equal(bits(m.a[k]), bits(v)), k


def test_plan_model_check_order(oracle):
    m, inp = _model(oracle)
    lo = np.zeros((5, 5), order="F")
    assert m.column_cond(0, lo) == PM.ESTATE                                    # never filled
    assert m.column_cond(3, lo) == PM.EINVAL and m.column_cond(0, None, None) == PM.EINVAL    # ... the arguments come first
    assert m.upload(inp) is None
    state = _state(m)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.column_cond(0, lo, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert m.column_cond(tc, lo) == PM.EINVAL, tc
    assert m.column_cond(0) == PM.EINVAL
    assert m.column_cond(0, lo, outs=()) == PM.EINVAL
    assert m.column_cond(0, lo, outs=("cover",)) == PM.EINVAL and m.column_cond(0, lo, outs=("mass", "kcnt")) == PM.EINVAL
    for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert m.column_cond(0, lo, None, first, ntr) == PM.EINVAL, (first, ntr)
        assert not isinstance(m.column_cond(0, lo, None, first, ntr, outs=("kcnt", "cover")), int)   # without cpath: not looked at
    # the order: the range, the handle, tc, the bounds, the outputs, the pairs, the tracers, the precision
    assert m.column_cond(9, None, None, 9, 9, sl0=0, n=0, outs=(), eb=4) == PM.EINVAL
    assert m.column_cond(0, lo, eb=4) == PM.ESTATE                              # a host form of the other precision
    assert m.column_cond(0, lo, None, 9, 9, eb=4) == PM.EINVAL and m.column_cond(9, lo, eb=4) == PM.EINVAL
    assert m.column_cond(0, lo, None, 9, 9, outs=("mass",), eb=4) == PM.EINVAL
    m.multi = True
    assert m.column_cond(0, lo) == PM.EUNSUPPORTED and m.column_cond(0, lo, sl0=0, n=0) == PM.EINVAL
    assert m.column_cond(9, None, None, 9, 9, outs=()) == PM.EUNSUPPORTED      # the handle comes before the rest
    m.multi = False
    assert _state(m) == state
    assert not isinstance(m.column_cond(1, lo, lo, 1, 1), int)                  # tc may be the value tracer


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.column_cond) and callable(mpdata.Plan.column_cond) and callable(mpdata.Plan.column_cond_host)
    for nm in ("column_cond", "column_cond_shapes"):
        assert nm in mpdata.__all__, nm


def test_column_cond_shapes(mpdata):
    assert mpdata.column_cond_shapes(5, 3, 8) == {"lo": (7, 5), "hi": (7, 5), "kcnt": (3, 5), "kbot": (3, 5), "ktop": (3, 5),
                                                 "cpath": (1, 3, 5), "cover": (5,), "mass": (1, 5)}
    sh = mpdata.column_cond_shapes(2, 65, 239, 3)
    assert sh["lo"] == (238, 2) and sh["kcnt"] == (65, 2) and sh["cpath"] == (3, 65, 2) and sh["mass"] == (3, 2) and sh["cover"] == (2,)


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def _arg_names(params):
    return [re.split(r"[\s*]+", p)[-1] for p in params]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3w." in hdr
    sec = hdr.split("---- 3w.")[1].split("---- 4.")[0]
    for word in ("tc", "lo", "hi", "kcnt", "kbot", "ktop", "cpath", "cover", "mass", "first_tracer", "nx", "MPDATA_EUNSUPPORTED",
                 "MPDATA_EINVAL", "MPDATA_ESTATE"):
        assert re.search(r"\b" + word + r"\b", sec), word
    # selection, windowed plans, the multi-GPU refusal
    assert "Selection means selection" in sec and "0 / 1 mask is" in sec and "contributes NOTHING" in sec
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec and "TALL level" in sec
    assert "mpdata_plan_shard_plan" in sec and "rounded ONCE" in sec and "compare-and-select" in sec
    assert "half-open" in sec and "(lo, hi]" in sec and "lo = +inf" in sec and "BAND" in sec
    for line in ("wgt(sl,k)    = rho(sl,k) * adz(sl,k)",
                 "in_k         = (lo ? c_k >  lo(b,k) : true)  and  (hi ? c_k <= hi(b,k) : true)",
                 "kcnt(b,i)    :  q = +0;  do k = 1, nzm:  if in_k:  q = q + 1",
                 "cpath(b,i,j) :  s = +0;  do k = 1, nzm:  if in_k:  s = s + wgt(sl,k) * v_k",
                 "cover(b)     :  q = +0;  do i = 1, nx:   if kcnt(b,i) > 0:  q = q + 1",
                 "mass(b,j)    :  s = +0;  do i = 1, nx:   s = s + cpath(b,i,j)"):
        assert line in sec, line
    assert "bits of 3k's path" in sec and "sum_i kcnt(b,i) == sum_k cnt(b,k)" in sec      # the two identities
    assert hdr.index("---- 3v.") < hdr.index("---- 3w.") < hdr.index("---- 4.")


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
    outs = ["kcnt", "kbot", "ktop", "cpath", "cover", "mass"]
    assert _arg_names(_c_params(hdr, "mpdata_plan_column_cond_device")) == \
        ["plan", "sl0", "n", "tc", "lo", "hi"] + outs + ["first_tracer", "ntracers"]
    for n in ("mpdata_plan_column_cond", "mpdata_plan_column_cond_f32"):
        assert _arg_names(_c_params(hdr, n)) == ["plan", "sl0", "n", "tc", "lo", "hi"] + outs
    for n in ("mpdata_column_cond_device", "mpdata_column_cond_f32_device"):
        assert _arg_names(_c_params(hdr, n)) == \
            ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "rho", "adz", "tc", "lo", "hi"] + outs + ["first_tracer", "ntr", "stream"]
        for i in (6, 7, 8, 10, 11):
            assert _c_params(hdr, n)[i].startswith("const ")                             # f, rho, adz, lo, hi are only read
    for i in (4, 5):
        assert _c_params(hdr, "mpdata_plan_column_cond_device")[i].startswith("const ")


# Fortran interface -> the C name it binds, a literal: the arrays are c_ptr, so each precision has an interface of its own
FORTRAN_IFACES = {
    "mpdata_plan_column_cond_device_c": "mpdata_plan_column_cond_device",
    "mpdata_plan_column_cond_c": "mpdata_plan_column_cond", "mpdata_plan_column_cond_f32_c": "mpdata_plan_column_cond_f32",
    "mpdata_column_cond_device_c": "mpdata_column_cond_device", "mpdata_column_cond_f32_device_c": "mpdata_column_cond_f32_device",
}


def test_fortran_interfaces_agree_with_the_header():
    """all five entry points, each bound by its literal name and public, the dummy arguments in the header's order, each of
    the header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    assert sorted(FORTRAN_IFACES.values()) == sorted(NAMES)
    for fname, cname in FORTRAN_IFACES.items():
        m = re.search(r"integer\(c_int\) function " + fname + r"\(([^)]*)\)\s*&?\s*bind\(C, name=\"" + cname +
                      r"\"\)(.*?)end function", f90, re.S)
        assert m, fname
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        params = _c_params(hdr, cname)
        cargs = _arg_names(params)
        assert fargs == cargs, (fargs, cargs)
        decl = {}
        for line in m.group(2).splitlines():
            d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\))\s*,\s*value\s*::\s*(.*)", line)
            if d:
                for a in d.group(2).split(","):
                    decl[a.strip()] = d.group(1)
        for p, a in zip(params, cargs):
            want = "type(c_ptr)" if "*" in p else "integer(c_int64_t)" if p.startswith("int64_t ") else "integer(c_int)"
            assert decl.get(a) == want, (fname, a, p, decl.get(a))
        assert re.search(r"public ::.*\b" + fname + r"\b", f90), fname
    # the fp32 entry points differ from the fp64 ones in the reals' type alone
    for c64, c32 in (("mpdata_plan_column_cond", "mpdata_plan_column_cond_f32"), ("mpdata_column_cond_device", "mpdata_column_cond_f32_device")):
        assert [p.replace("float", "double") for p in _c_params(hdr, c32)] == _c_params(hdr, c64)
    # in the second interface block, behind 3v's binding
    assert f90.index("mpdata_plan_level_cond_device_c(plan") < f90.index("mpdata_plan_column_cond_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert f90.rindex("\n  interface\n") < f90.index("mpdata_plan_column_cond_device_c(plan")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "column_cond_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\bcolumn_cond\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, rho, adz, tc, the bounds, the outputs, the
    pairs, the tracers"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    for fn in (L.mpdata_column_cond_device, L.mpdata_column_cond_f32_device):
        def call(ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, rho=one, adz=one, tc=0, lo=one, hi=None, kcnt=one, kbot=None, ktop=None,
                 cpath=one, cover=None, mass=None, first=0, ntr=3):
            return fn(ncrms, nx, nz, T, sl0, n, f, rho, adz, tc, lo, hi, kcnt, kbot, ktop, cpath, cover, mass, first, ntr, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        assert call(rho=None) == mpdata.EINVAL and b"null rho" in err()
        assert call(adz=None) == mpdata.EINVAL and b"null adz" in err()
        for tc in (-1, 3):
            assert call(tc=tc) == mpdata.EINVAL and b"condition tracer" in err(), tc
        assert call(lo=None) == mpdata.EINVAL and b"lo and hi are both NULL" in err()
        assert call(kcnt=None, cpath=None) == mpdata.EINVAL and b"every output is NULL" in err()
        assert call(kcnt=None, cover=one) == mpdata.EINVAL and b"cover without kcnt" in err()
        assert call(cpath=None, mass=one) == mpdata.EINVAL and b"mass without cpath" in err()
        for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1), (2147483647, 2)):
            assert call(first=first, ntr=ntr) == mpdata.EINVAL and b"tracer range" in err(), (first, ntr)
        # the order: each refusal hides the ones behind it
        bad = dict(tc=9, lo=None, kcnt=None, cpath=None, ntr=9)
        assert call(nz=1, sl0=9, f=None, **bad) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, **bad) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, **bad) == mpdata.EINVAL and b"null f" in err()
        assert call(**bad) == mpdata.EINVAL and b"condition tracer" in err()
        assert call(**dict(bad, tc=0)) == mpdata.EINVAL and b"lo and hi" in err()
        assert call(**dict(bad, tc=0, lo=one)) == mpdata.EINVAL and b"every output" in err()
        assert call(**dict(bad, tc=0, lo=one, cover=one)) == mpdata.EINVAL and b"cover without kcnt" in err()
        assert call(kcnt=None, mass=one, ntr=9) == mpdata.EINVAL and b"tracer range" in err()
    dev = lambda plan=one, sl0=0, n=1, tc=0, lo=one, kcnt=one: \
        L.mpdata_plan_column_cond_device(plan, sl0, n, tc, lo, None, kcnt, None, None, None, None, None, 0, 0)
    assert dev(plan=None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_column_cond(None, 0, 1, 0, one, None, one, None, None, None, None, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_column_cond_f32(None, 0, 1, 0, one, None, one, None, None, None, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert dev(sl0=sl0, n=n) == mpdata.EINVAL
    assert dev(n=0, tc=9, lo=None, kcnt=None) == mpdata.EINVAL and b"n = 0" in err()     # the range came first


def test_new_kernels_do_not_spill_and_use_no_scratch():
    """the resource-usage report the build writes next to the object of mpdata_column_cond.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel.  The register arrays of the plan-layout kernel (the in-bits, the running
    sums of a windowed plan) rotate through position 0, so none is indexed at run time and none lives in memory; its
    arguments go through LDS once and the presence of lo and hi is a template parameter, so the scalar registers hold the
    nest.  Kernels: the plan-layout one for double and float2 elements, plain and windowed, with lo, with hi and with both
    (12); the reference-layout one and the cover / mass kernel for double and float.  The file has no inline assembly and is
    built without contraction."""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_column_cond.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_column_cond_kernel", txt)) == 12
    assert len(re.findall(r"Function Name: \S*ref_column_cond_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*column_cond_tail_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 16 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_column_cond.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "asm" not in code and "__syncthreads" in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_column_cond\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_column_cond", mk)
    assert "mpdata_column_cond$(O)" in mk.split("OBJS :=")[1].split("\n")[0]
    assert "mpdata_column_cond.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
