"""Tests without a GPU of the per-level histograms (include/mpdata_hip.h 3ab): the numpy model of
tests/level_hist_model.py against tests/level_cond_model.py bin by bin, the edge rules, the variants the GPU tests must tell
apart, the plan model's check order, and the interface -- the header section, the prototype table of capi.py, the Fortran
module, the argument checks that need no device and the resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import level_cond_model as LC
import level_hist_model as LH
from oracle import plan_model as PM
from test_plan_level_hist import KINDS, NBS, SEED, TRIPLES
from test_plan_level_hist_sequences import CASES
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_hist_device", "mpdata_plan_level_hist", "mpdata_plan_level_hist_f32", "mpdata_level_hist_device",
         "mpdata_level_hist_f32_device")
DTYPES = [np.float64, np.float32]
SHAPES = sorted({(k[0], np.dtype(k[2]).name) for k in KINDS.values()} | {(c[1], np.dtype(c[3]).name) for c in CASES})
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{d}" for s, d in SHAPES]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 2, (n, nx + 6, nz - 1, T))
    return np.asfortranarray(np.where(rng.integers(0, 2, f.shape) == 0, np.round(f * 8) / 8, f).astype(dtype))


# ---- the model against level_cond's, bin by bin, on every shape and bin count of the GPU tests
@pytest.mark.parametrize("shape,dtn", SHAPES, ids=IDS)
def test_every_bin_has_the_bits_of_level_cond(oracle, shape, dtn):
    dt = np.dtype(dtn).type
    F = LH.make_plan_inputs(oracle, shape, 3, dt, SEED)["f"]
    n, nzm = F.shape[0], F.shape[2]
    for j, nb in enumerate(NBS):
        tc, first, ntr = TRIPLES[j % 4]
        e = LH.call_edges(nb, 4 * j)                           # finite ends
        cnt, bsum = LH.level_hist(F, tc, e, nb, first, ntr)
        assert cnt.shape == (n, nzm, nb) and bsum.shape == (n, nzm, nb, ntr) and cnt.dtype == dt and bsum.dtype == dt
        for b in range(nb):
            lo, hi = (np.full((n, nzm), dt(e[k]), dt, order="F") for k in (b, b + 1))
            q, s = LC.level_cond(F, tc, lo, hi, first, ntr)
            assert same(np.asfortranarray(cnt[:, :, b]), q) and same(np.asfortranarray(bsum[:, :, b]), s), (nb, b)
        assert (cnt.sum(axis=2) <= shape[1]).all()


# ---- the edge rules
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rules(dtype):
    dt = np.dtype(dtype).type
    F = field(3, 9, 6, 2, dtype, 5)
    nx = 9
    # equal neighbouring edges: an empty bin, and the others as without the repeat
    cnt, bsum = LH.level_hist(F, 0, [-1, 0.5, 0.5, 2], 3, 0, 2)
    c2, s2 = LH.level_hist(F, 0, [-1, 0.5, 2], 2, 0, 2)
    assert not cnt[:, :, 1].any() and not bsum[:, :, 1].any() and not np.signbit(bsum[:, :, 1]).any()
    assert same(np.asfortranarray(cnt[:, :, [0, 2]]), c2) and same(np.asfortranarray(bsum[:, :, [0, 2]]), s2)
    # -inf / +inf ends collect everything; finite ends leave c <= e_0 and c > e_nb out
    cnt = LH.level_hist(F, 0, [-np.inf, 0, 1, np.inf], 3, 0, 0)[0]
    assert (cnt.sum(axis=2) == nx).all()
    c = F[:, 3:nx + 3, :, 0]
    cnt = LH.level_hist(F, 0, [0, 0.5, 1], 2, 0, 0)[0]
    assert np.array_equal(cnt.sum(axis=2), ((c > 0) & (c <= 1)).sum(axis=1)) and ((c == 0).any() and (c == 1).any())
    # an edge belongs to the bin below: c == e_j is in bin j - 1
    G = np.array(F)
    G[:, 3:nx + 3, :, 0] = dt(0.5)
    cnt = LH.level_hist(G, 0, [0, 0.5, 1], 2, 0, 0)[0]
    assert (cnt[:, :, 0] == nx).all() and not cnt[:, :, 1].any()
    # -0.0 against an edge of 0: equal, so not above it
    G[:, 3:nx + 3, :, 0] = dt(-0.0)
    cnt = LH.level_hist(G, 0, [-1, 0, 1], 2, 0, 0)[0]
    assert (cnt[:, :, 0] == nx).all() and not cnt[:, :, 1].any()
    assert not LH.level_hist(G, 0, [0.0, 1], 1, 0, 0)[0].any() and not LH.level_hist(G, 0, [-0.0, 1], 1, 0, 0)[0].any()
    # a NaN in tc is in no bin, with infinite ends too
    N = LH.plant_nan(F, 0)
    cnt, bsum = LH.level_hist(N, 0, [-np.inf, 0.5, np.inf], 2, 1, 1)
    assert np.array_equal(cnt.sum(axis=2), nx - np.isnan(N[:, 3:nx + 3, :, 0]).sum(axis=1)) and np.isnan(N[..., 0]).any()
    assert np.isfinite(bsum).all()
    # ... but as a VALUE of a column that is in a bin it is summed
    assert np.isnan(LH.level_hist(N, 1, [-np.inf, np.inf], 1, 0, 1)[1]).any()
    # inf or NaN in an excluded cell of a value tracer reaches no sum; a multiplied mask lets it in
    e = [-0.5, 0.25, 1.5]
    P = LH.plant(F, 0, e, 2, 1)
    assert np.isnan(P[..., 1]).any() and np.isposinf(P[..., 1]).any()
    assert np.isfinite(LH.level_hist(P, 0, e, 2, 0, 2)[1]).all()
    assert not np.isfinite(LH.level_hist(P, 0, e, 2, 1, 1, multiply=True)[1]).all()
    # the edges are rounded once to the field's precision
    if dtype == np.float32:
        third = 1 / 3
        G[:, 3:nx + 3, :, 0] = np.float32(third)               # > 1/3 as a double, == the rounded edge
        assert not LH.level_hist(G, 0, [third, 1], 1, 0, 0)[0].any()


# ---- the shapes of the GPU tests: the inputs tell the variants apart
@pytest.mark.parametrize("shape,dtn", SHAPES, ids=IDS)
def test_inputs_tell_the_variants_apart(oracle, shape, dtn):
    """on the field the GPU tests upload, over their four triples and bin counts 5, 17 and 32 with the edges of
    LH.call_edges: >= for >, a bin index off by one, the edge of the wrong bin, a mask multiplied in (on a planted field)
    and a NaN counted in bin 0 (on a field with NaNs planted) each change at least one output row in ten, the reversed walk
    at least one row of sums in ten where one or two bins hold every column -- but at nx = 2, where the reversed sum of two
    terms is the same sum"""
    ncrms, nx, nz = shape
    F = LH.make_plan_inputs(oracle, shape, 3, np.dtype(dtn).type, SEED)["f"]
    assert (F < 0).any() and (F > 0).any()
    s = LH.variant_shares(F, TRIPLES, (5, 17, 32))
    for v in ("ge", "off", "edge", "multiply", "nan0"):
        assert s[v] >= 0.1, (v, s)
    assert s["reverse"] == 0 if nx == 2 else s["reverse"] >= 0.1, s


# ---- the plan model: the call changes nothing; the order of the checks
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = LH.PlanModelLevelHist(oracle, *shape, T, dtype)
    return m, LH.make_plan_inputs(oracle, shape, T, dtype, 100)


def _state(m):
    return (m.boundary, m.uploaded, m.have_u, m.have_w, m.timing, m.ran, list(m.steps), list(m.fmax), list(m.flmax))


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_call_changes_no_array_and_no_mark(oracle, boundary):
    m, inp = _model(oracle)
    assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None
    keep, state = {k: np.array(v) for k, v in m.a.items()}, _state(m)
    for j, (tc, first, ntr) in enumerate(TRIPLES):
        nb = NBS[2 * j + 1]
        e = LH.sample_edges(keep["f"][1:4], tc, nb, 5)
        for kw in (dict(), dict(cnt=False), dict(bsum=False)):
            cnt, bsum = m.level_hist(tc, e, nb, first, ntr, sl0=1, n=3, **kw)
            want = LH.level_hist(keep["f"][1:4], tc, e, nb, first, ntr)
            assert (cnt is None) == (kw.get("cnt") is False) and (bsum is None) == (kw.get("bsum") is False)
            assert cnt is None or (same(cnt, want[0]) and cnt.shape == (3, 5, nb))
            assert bsum is None or (same(bsum, want[1]) and bsum.shape == (3, 5, nb, ntr))
            assert _state(m) == state
            for k, v in keep.items():
                assert np.array_equal(bits(m.a[k]), bits(v)), k


def test_plan_model_check_order(oracle):
    """the error list of 3ab and its order"""
    m, inp = _model(oracle)
    e = [0.0, 0.5, 1.0]
    nan, desc = [0.0, float("nan"), 1.0], [0.0, 1.0, 0.5]
    assert m.level_hist(0, e) == PM.ESTATE                                      # never filled
    assert m.level_hist(3, e) == PM.EINVAL and m.level_hist(0, None) == PM.EINVAL            # ... the arguments come first
    assert m.upload(inp) is None
    state = _state(m)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.level_hist(0, e, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert m.level_hist(tc, e) == PM.EINVAL, tc
    for nb in (0, -1, 33):
        assert m.level_hist(0, [0.0] * 40, nb) == PM.EINVAL, nb
    assert not isinstance(m.level_hist(0, [0.0] * 40, 32), int) and not isinstance(m.level_hist(0, e, 1), int)
    assert m.level_hist(0, None, 2) == PM.EINVAL and m.level_hist(0, nan) == PM.EINVAL and m.level_hist(0, desc) == PM.EINVAL
    assert not isinstance(m.level_hist(0, desc, 1), int)                        # (only the nb + 1 edges of the call are looked at)
    assert not isinstance(m.level_hist(0, [-np.inf, 0.0, 0.0, np.inf]), int)    # equal edges and infinite ends are fine
    assert m.level_hist(0, e, cnt=False, bsum=False) == PM.EINVAL
    for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert m.level_hist(0, e, 2, first, ntr) == PM.EINVAL, (first, ntr)
        assert not isinstance(m.level_hist(0, e, 2, first, ntr, bsum=False), int)            # without bsum: not looked at
    # the order: the range, the handle, tc, nb, the edges, the outputs, the tracers, the precision, the state
    assert m.level_hist(9, None, 0, 9, 9, sl0=0, n=0, cnt=False, bsum=False, eb=4) == PM.EINVAL
    assert m.level_hist(0, e, eb=4) == PM.ESTATE                                # a host form of the other precision
    assert m.level_hist(0, e, 2, 9, 9, eb=4) == PM.EINVAL and m.level_hist(9, e, eb=4) == PM.EINVAL
    assert m.level_hist(0, nan, eb=4) == PM.EINVAL and m.level_hist(0, e, 33, eb=4) == PM.EINVAL
    m.multi = True
    assert m.level_hist(0, e) == PM.EUNSUPPORTED and m.level_hist(0, e, sl0=0, n=0) == PM.EINVAL
    assert m.level_hist(9, None, 0, 9, 9, cnt=False, bsum=False) == PM.EUNSUPPORTED          # the handle comes before the rest
    m.multi = False
    assert _state(m) == state
    assert not isinstance(m.level_hist(1, e, 2, 1, 1), int)                     # tc may be the value tracer


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.level_hist) and callable(mpdata.Plan.level_hist) and callable(mpdata.Plan.level_hist_host)
    for nm in ("level_hist", "level_hist_shapes", "LEVEL_HIST_MAX_BINS"):
        assert nm in mpdata.__all__, nm
    assert mpdata.LEVEL_HIST_MAX_BINS == 32 == LH.MAX_BINS
    assert mpdata.level_hist_shapes(5, 3, 8, 4) == {"cnt": (4, 7, 5), "bsum": (1, 4, 7, 5)}
    assert mpdata.level_hist_shapes(2, 65, 239, 32, 3) == {"cnt": (32, 238, 2), "bsum": (3, 32, 238, 2)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3ab." in hdr
    sec = hdr.split("---- 3ab.")[1].split("---- 4.")[0]
    for word in ("tc", "nb", "edges", "cnt", "bsum", "first_tracer", "nx", "MPDATA_EUNSUPPORTED", "MPDATA_EINVAL", "MPDATA_ESTATE",
                 "MPDATA_LEVEL_HIST_MAX_BINS", "HOST"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert re.search(r"#define MPDATA_LEVEL_HIST_MAX_BINS 32\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "half-open" in sec and "(e_j, e_{j+1}]" in sec and "NaN in c_i is INSIDE the contract" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec and "compare-and-select" in sec
    for line in ("e_j = edges[j] rounded once to the plan's precision          j = 0 .. nb",
                 "m_i = the number of j in 0 .. nb with c_i > e_j              (0 .. nb + 1)",
                 "column i is in bin j = m_i - 1 when 1 <= m_i <= nb, else in no bin",
                 "cnt(b,k,j)    :  q = +0;  do i = 1, nx:  if column i in bin j:  q = q + 1",
                 "bsum(b,k,j,r) :  s = +0;  do i = 1, nx:  if column i in bin j:  s = s + v_i     (r = t - first_tracer)"):
        assert line in sec, line
    assert hdr.index("---- 3aa.") < hdr.index("---- 3ab.") < hdr.index("---- 4.")


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
    names = lambda n: [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)]
    assert names("mpdata_plan_level_hist_device") == ["plan", "sl0", "n", "tc", "nb", "edges", "cnt", "bsum", "first_tracer", "ntracers"]
    assert names("mpdata_plan_level_hist") == names("mpdata_plan_level_hist_f32") == ["plan", "sl0", "n", "tc", "nb", "edges", "cnt", "bsum"]
    assert names("mpdata_level_hist_device") == names("mpdata_level_hist_f32_device") == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "tc", "nb", "edges", "cnt", "bsum", "first_tracer", "ntr", "stream"]
    assert _c_params(hdr, "mpdata_level_hist_device")[6].startswith("const ")       # f is only read
    for n in NAMES:                                          # edges: doubles on the host in every form
        assert [p for p in _c_params(hdr, n) if p.endswith("edges")] == ["const double* edges"], n


@pytest.mark.parametrize("name", NAMES)
def test_fortran_interface_agrees_with_the_header(name):
    """every interface, bound by the literal name, public, the dummy arguments in the header's order, each of the header's
    kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function " + name + r"_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"" + name + r"\"\)(.*?)end function",
                  f90, re.S)
    assert m
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
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert re.search(r"public ::.*\b" + name + r"_c\b", f90)
    # in the second interface block, behind 3aa's bindings
    assert f90.index("mpdata_column_scan_f32_device_c(ncrms") < f90.index(name + "_c(")
    assert f90.count("\n  interface\n") == 2 and f90.rindex("\n  interface\n") < f90.index(name + "_c(")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "level_hist_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\blevel_hist\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, tc, nb, the edges, the outputs, the tracers"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    arr = lambda a: ctypes.cast((ctypes.c_double * len(a))(*a), ctypes.c_void_p)
    ok, nan, desc, eq = arr([0, 1, 2, 3]), arr([0, float("nan"), 2, 3]), arr([0, 2, 1, 3]), arr([0, 0, 0, 0])
    for fn in (L.mpdata_level_hist_device, L.mpdata_level_hist_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, tc=0, nb=3, e=ok, cnt=one, bsum=one, first=0, ntr=3: \
            fn(ncrms, nx, nz, T, sl0, n, f, tc, nb, e, cnt, bsum, first, ntr, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        for tc in (-1, 3):
            assert call(tc=tc) == mpdata.EINVAL and b"binned tracer" in err(), tc
        for nb in (0, -3, 33):
            assert call(nb=nb) == mpdata.EINVAL and b"outside [1, 32]" in err(), nb
        assert call(e=None) == mpdata.EINVAL and b"null edges" in err()
        assert call(e=nan) == mpdata.EINVAL and b"edges[1] is a NaN" in err()
        assert call(e=desc) == mpdata.EINVAL and b"edges[1] > edges[2]" in err()
        assert call(e=desc, nb=1, cnt=None, bsum=None) == mpdata.EINVAL and b"both NULL" in err()   # (edges beyond nb: not looked at)
        assert call(e=eq, cnt=None, bsum=None) == mpdata.EINVAL and b"both NULL" in err()           # (equal edges are fine)
        for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1), (2147483647, 2)):
            assert call(first=first, ntr=ntr) == mpdata.EINVAL and b"tracer range" in err(), (first, ntr)
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, tc=9, nb=0, e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, tc=9, nb=0, e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, tc=9, nb=0, e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"null f" in err()
        assert call(tc=9, nb=0, e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"binned tracer" in err()
        assert call(nb=0, e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"nb 0" in err()
        assert call(e=None, cnt=None, bsum=None) == mpdata.EINVAL and b"null edges" in err()
        assert call(e=nan, cnt=None, bsum=None) == mpdata.EINVAL and b"NaN" in err()
        assert call(cnt=None, bsum=None, ntr=9) == mpdata.EINVAL and b"cnt and bsum" in err()
        assert call(cnt=None, ntr=9) == mpdata.EINVAL and b"tracer range" in err()
    dev = lambda plan=one, sl0=0, n=1, tc=0, e=ok, cnt=one: L.mpdata_plan_level_hist_device(plan, sl0, n, tc, 3, e, cnt, None, 0, 0)
    assert dev(plan=None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_hist(None, 0, 1, 0, 3, ok, one, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_hist_f32(None, 0, 1, 0, 3, ok, one, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert dev(sl0=sl0, n=n) == mpdata.EINVAL
    assert dev(n=0, tc=9, e=None, cnt=None) == mpdata.EINVAL and b"n = 0" in err()     # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_level_hist.hip: no scratch memory, no vector
    and no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS and has no barrier and
    no atomic.  Kernels: the plan-layout one for the bin classes 4 and 8 with double and float2 elements and 16 with double
    alone, the reference-layout one (class 8) for double and float."""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_level_hist.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_level_hist_kernel", txt)) == 5
    assert len(re.findall(r"Function Name: \S*ref_level_hist_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 7 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_level_hist.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "atomic" not in code and "#ifndef" not in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_level_hist\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_level_hist", mk)
    assert "mpdata_level_hist$(O)" in mk.split("OBJS :=")[1].split("\n")[0]
    assert "mpdata_level_hist.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
