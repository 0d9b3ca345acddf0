"""CPU tests of the per-level conditional counts and sums (include/mpdata_hip.h 3v): the numpy model of
tests/level_cond_model.py against a plain-Python triple loop and against what the definition implies -- the bins (lo, hi]
tile the line, an empty level gives +0 and a full one nx, no sum is ever -0, an excluded infinity or NaN reaches no sum --,
the shares in which the variants that are NOT the definition differ from it at every shape the GPU tests run, the plan
model's rules, and the interface (header, ctypes, Fortran, Python names, the argument checks that need no device, the
compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import level_cond_model as LC
from oracle import plan_model as PM
from test_plan_level_cond import KINDS, SEED, TRIPLES
from test_plan_level_cond_sequences import CASES
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_cond_device", "mpdata_plan_level_cond", "mpdata_plan_level_cond_f32", "mpdata_level_cond_device",
         "mpdata_level_cond_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    return np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, T)).astype(dtype))


def same(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)))


# ---- the model against the definition
@pytest.mark.parametrize("bounds", LC.BOUNDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_plain_triple_loop(dtype, bounds):
    n, nx, nz, T = 3, 5, 11, 3
    f = field(n, nx, nz, T, dtype, 11)
    f[:, :3] = f[:, nx + 3:] = np.nan                       # halo columns are not read
    for tc, first, ntr in TRIPLES + ((0, 0, 0),):
        lo, hi = LC.call_args(f, tc, bounds, 12 + tc)
        got = LC.level_cond(f, tc, lo, hi, first, ntr)
        want = LC.level_cond_loops(f, tc, lo, hi, first, ntr)
        assert same(got[0], want[0]) and same(got[1], want[1]) and got[0].dtype == dtype
        assert np.isfinite(got[0]).all() and (ntr == 0 or np.isfinite(got[1]).all())
        assert got[0].shape == (n, nz - 1) and (ntr == 0 or got[1].shape == (n, nz - 1, ntr))
        g = np.array(f)
        g[..., [t for t in range(T) if t != tc and not first <= t < first + ntr]] = np.nan      # ... and no other tracer
        assert same(LC.level_cond(g, tc, lo, hi, first, ntr)[1], got[1])
        # the drawn bounds: the ties exist in every row that is neither empty nor full; one row in five of each
        c = f[:, 3:nx + 3, :, tc]
        kind = np.add.outer(np.arange(n), np.arange(nz - 1)) % 5
        assert (got[0][kind == 0] == 0).all() and (got[0][kind == 1] == nx).all()
        mid = kind >= 2
        if lo is not None:
            assert ((c == lo[:, None]).any(axis=1) | ~mid).all()
        if hi is not None:
            assert ((c == hi[:, None]).any(axis=1) | ~mid).all()
        assert lo is None or (got[0][mid] < nx).all()        # the column of lo is out
        assert hi is None or (got[0][mid] >= 1).all()        # the column of hi is in


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bins_tile_the_line_and_edges_belong_to_the_bin_below(dtype):
    """(lo, hi]: with edges that are values of the field, cnt of (e0, e1] plus cnt of (e1, e2] is cnt of (e0, e2] and the
    three bins (-inf, e1], (e1, e2], (e2, +inf) hold every column once"""
    n, nx, nz, T = 4, 9, 8, 3
    f = field(n, nx, nz, T, dtype, 21)
    c = np.sort(f[:, 3:nx + 3, :, 1], axis=1)
    e0, e1, e2 = (np.asfortranarray(c[:, i]) for i in (1, 4, 7))
    cnt = lambda lo, hi: LC.level_cond(f, 1, lo, hi, 0, 0)[0]
    assert np.array_equal(cnt(e0, e1) + cnt(e1, e2), cnt(e0, e2)) and (cnt(e0, e1) == 3).all()
    assert (cnt(None, e1) + cnt(e1, e2) + cnt(e2, None) == nx).all()
    assert (cnt(None, e1) == 5).all() and (cnt(e2, None) == 1).all()        # the edge itself lies in the bin below
    assert (cnt(e1, e1) == 0).all() and (cnt(e2, e0) == 0).all()            # lo >= hi: empty
    z = LC.level_cond(f, 1, e2, e0, 0, 3)
    assert not z[0].any() and not z[1].any() and not np.signbit(z[0]).any() and not np.signbit(z[1]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_sum_is_never_negative_zero_so_a_selected_zero_may_be_added(dtype):
    """s starts at +0 and x + y is -0 only for x = y = -0, so no s is -0: adding a selected +0 for an excluded column keeps
    every bit, which is what allows a kernel to select the term instead of the sum -- also where the field holds -0.0"""
    n, nx, nz, T = 3, 6, 9, 3
    f = field(n, nx, nz, T, dtype, 31)
    f[:, 3::2, :, 2] = dtype(-0.0)
    f[0, :, :, 0] = dtype(-0.0)
    lo, hi = LC.call_args(f, 1, "both", 32)
    cnt, csum = LC.level_cond(f, 1, lo, hi, 0, 3)
    assert not np.signbit(csum[csum == 0]).any() and (csum == 0).any() and not np.signbit(cnt).any()
    # the term selected (v or +0) and always added: the same bits
    s = np.zeros_like(csum)
    c = f[:, 3:nx + 3, :, 1]
    for i in range(nx):
        inn = (c[:, i] > lo) & (c[:, i] <= hi)
        s = s + np.where(inn[..., None], f[:, 3 + i], dtype(0))
    assert same(np.asfortranarray(s), csum)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_excluded_infinities_and_nans_reach_no_sum_but_a_multiplied_mask_lets_them_in(dtype):
    n, nx, nz, T = 5, 7, 12, 3
    f = field(n, nx, nz, T, dtype, 41)
    for tc, t, bounds in ((0, 2, "both"), (2, 1, "lo"), (1, 0, "hi")):
        lo, hi = LC.call_args(f, tc, bounds, 42)
        P = LC.plant(f, tc, lo, hi, t)
        assert np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        cnt, csum = LC.level_cond(P, tc, lo, hi, 0, T)
        assert np.isfinite(csum).all() and same(cnt, LC.level_cond(f, tc, lo, hi, 0, T)[0])
        assert same(csum, LC.level_cond(f, tc, lo, hi, 0, T)[1])               # ... as if nothing had been planted
        bad = LC.level_cond(P, tc, lo, hi, t, 1, multiply=True)[1]
        assert np.isnan(bad[cnt < nx]).all() and np.isfinite(bad[cnt == nx]).all()
    # on a finite field the multiplied mask is the definition, bit for bit: only a planted field tells it apart
    lo, hi = LC.call_args(f, 0, "both", 43)
    assert same(LC.level_cond(f, 0, lo, hi, 0, T, multiply=True)[1], LC.level_cond(f, 0, lo, hi, 0, T)[1])


# ---- the shapes of the GPU tests: the drawn inputs tell the variants apart
SHAPES = sorted({(k[0], np.dtype(k[2]).name) for k in KINDS.values()} | {(c[1], np.dtype(c[3]).name) for c in CASES})


@pytest.mark.parametrize("shape,dtn", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{d}" for s, d in SHAPES])
def test_drawn_inputs_tell_the_variants_apart(oracle, shape, dtn):
    """on the field the GPU tests upload, over their four triples with both bounds: >= for >, < for <= and a mask
    multiplied in (on a planted field) each change at least one output in ten, lo of the level below at least one in ten
    (nz = 8: one in fifty is asked for), the reversed walk at least one sum in ten -- but at nx = 2, where the reversed sum
    of two terms is the same sum"""
    ncrms, nx, nz = shape
    F = LC.make_plan_inputs(oracle, shape, 3, np.dtype(dtn).type, SEED)["f"]
    assert (F < 0).any() and (F > 0).any()
    s = LC.variant_shares(F, TRIPLES)
    assert s["ge"] >= 0.1 and s["lt"] >= 0.1 and s["multiply"] >= 0.1, s
    assert s["shift"] >= (0.02 if nz == 8 else 0.1), s
    assert s["reverse"] == 0 if nx == 2 else s["reverse"] >= 0.1, s


# ---- the plan model: the call changes nothing; the order of the checks
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = LC.PlanModelLevelCond(oracle, *shape, T, dtype)
    return m, LC.make_plan_inputs(oracle, shape, T, dtype, 100)


def _state(m):
    return (m.boundary, m.uploaded, m.have_u, m.have_w, m.timing, m.ran, list(m.steps), list(m.fmax), list(m.flmax))


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_call_changes_no_array_and_no_mark(oracle, boundary):
    m, inp = _model(oracle)
    assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None
    keep, state = {k: np.array(v) for k, v in m.a.items()}, _state(m)
    for tc, first, ntr in TRIPLES:
        for bounds in LC.BOUNDS:
            lo, hi = LC.call_args(keep["f"][1:4], tc, bounds, 5)
            for kw in (dict(), dict(cnt=False), dict(csum=False)):
                cnt, csum = m.level_cond(tc, lo, hi, first, ntr, sl0=1, n=3, **kw)
                want = LC.level_cond(keep["f"][1:4], tc, lo, hi, first, ntr)
                assert (cnt is None) == (kw.get("cnt") is False) and (csum is None) == (kw.get("csum") is False)
                assert cnt is None or (same(cnt, want[0]) and cnt.shape == (3, 5))
                assert csum is None or (same(csum, want[1]) and csum.shape == (3, 5, ntr))
                assert _state(m) == state
                for k, v in keep.items():
                    assert np.array_equal(bits(m.a[k]), bits(v)), k


def test_plan_model_check_order(oracle):
    m, inp = _model(oracle)
    lo = np.zeros((5, 5), order="F")
    assert m.level_cond(0, lo) == PM.ESTATE                                     # never filled
    assert m.level_cond(3, lo) == PM.EINVAL and m.level_cond(0, None, None) == PM.EINVAL     # ... the arguments come first
    assert m.upload(inp) is None
    state = _state(m)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.level_cond(0, lo, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert m.level_cond(tc, lo) == PM.EINVAL, tc
    assert m.level_cond(0) == PM.EINVAL
    assert m.level_cond(0, lo, cnt=False, csum=False) == PM.EINVAL
    for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert m.level_cond(0, lo, None, first, ntr) == PM.EINVAL, (first, ntr)
        assert not isinstance(m.level_cond(0, lo, None, first, ntr, csum=False), int)         # without csum: not looked at
    # the order: the range, the handle, tc, the bounds, the outputs, the tracers, the precision
    assert m.level_cond(9, None, None, 9, 9, sl0=0, n=0, cnt=False, csum=False, eb=4) == PM.EINVAL
    assert m.level_cond(0, lo, eb=4) == PM.ESTATE                               # a host form of the other precision
    assert m.level_cond(0, lo, None, 9, 9, eb=4) == PM.EINVAL and m.level_cond(9, lo, eb=4) == PM.EINVAL
    m.multi = True
    assert m.level_cond(0, lo) == PM.EUNSUPPORTED and m.level_cond(0, lo, sl0=0, n=0) == PM.EINVAL
    assert m.level_cond(9, None, None, 9, 9, cnt=False, csum=False) == PM.EUNSUPPORTED   # the handle comes before the rest
    m.multi = False
    assert _state(m) == state
    assert not isinstance(m.level_cond(1, lo, lo, 1, 1), int)                   # tc may be the value tracer


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.level_cond) and callable(mpdata.Plan.level_cond) and callable(mpdata.Plan.level_cond_host)
    for nm in ("level_cond", "level_cond_shapes"):
        assert nm in mpdata.__all__, nm


def test_level_cond_shapes(mpdata):
    assert mpdata.level_cond_shapes(5, 3, 8) == {"lo": (7, 5), "hi": (7, 5), "cnt": (7, 5), "csum": (1, 7, 5)}
    assert mpdata.level_cond_shapes(2, 65, 239, 3) == {"lo": (238, 2), "hi": (238, 2), "cnt": (238, 2), "csum": (3, 238, 2)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3v." in hdr
    sec = hdr.split("---- 3v.")[1].split("---- 4.")[0]
    for word in ("tc", "lo", "hi", "cnt", "csum", "first_tracer", "nx", "MPDATA_EUNSUPPORTED", "MPDATA_EINVAL", "MPDATA_ESTATE"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert "-0" in sec and "s + (+0) keeps every bit" in sec and "0 / 1 mask is therefore wrong" in sec
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec
    assert "half-open" in sec and "(lo, hi]" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec and "compare-and-select" in sec
    for line in ("in_i = (lo ? c_i >  lo(b,k) : true)  and  (hi ? c_i <= hi(b,k) : true)",
                 "cnt(b,k)    :  q = +0;  do i = 1, nx:  if in_i:  q = q + 1",
                 "csum(b,k,j) :  s = +0;  do i = 1, nx:  if in_i:  s = s + v_i"):
        assert line in sec, line
    assert hdr.index("---- 3u.") < hdr.index("---- 3v.") < hdr.index("---- 4.")


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
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_level_cond_device")] == \
        ["plan", "sl0", "n", "tc", "lo", "hi", "cnt", "csum", "first_tracer", "ntracers"]
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_level_cond")] == \
        ["plan", "sl0", "n", "tc", "lo", "hi", "cnt", "csum"]
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_level_cond_device")] == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "tc", "lo", "hi", "cnt", "csum", "first_tracer", "ntr", "stream"]
    assert _c_params(hdr, "mpdata_level_cond_device")[6].startswith("const ")       # f is only read
    for i in (4, 5):
        assert _c_params(hdr, "mpdata_plan_level_cond_device")[i].startswith("const ")


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_level_cond_device_c\(([^)]*)\)\s*&?\s*"
                  r"bind\(C, name=\"mpdata_plan_level_cond_device\"\)(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_level_cond_device")
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
    assert re.search(r"public ::.*\bmpdata_plan_level_cond_device_c\b", f90)
    # in the second interface block, behind 3u's binding
    assert f90.index("mpdata_plan_level_cov_device_c(plan") < f90.index("mpdata_plan_level_cond_device_c(plan")
    assert f90.count("\n  interface\n") == 2
    assert f90.rindex("\n  interface\n") < f90.index("mpdata_plan_level_cond_device_c(plan")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "level_cond_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\blevel_cond\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, f, tc, the bounds, the outputs, the tracers"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    for fn in (L.mpdata_level_cond_device, L.mpdata_level_cond_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, tc=0, lo=one, hi=None, cnt=one, csum=one, first=0, ntr=3: \
            fn(ncrms, nx, nz, T, sl0, n, f, tc, lo, hi, cnt, csum, first, ntr, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        for tc in (-1, 3):
            assert call(tc=tc) == mpdata.EINVAL and b"condition tracer" in err(), tc
        assert call(lo=None) == mpdata.EINVAL and b"lo and hi are both NULL" in err()
        assert call(cnt=None, csum=None) == mpdata.EINVAL and b"cnt and csum are both NULL" in err()
        for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1), (2147483647, 2)):
            assert call(first=first, ntr=ntr) == mpdata.EINVAL and b"tracer range" in err(), (first, ntr)
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, f=None, tc=9, lo=None, cnt=None, csum=None) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, f=None, tc=9, lo=None, cnt=None, csum=None) == mpdata.EINVAL and b"outside" in err()
        assert call(f=None, tc=9, lo=None, cnt=None, csum=None) == mpdata.EINVAL and b"null f" in err()
        assert call(tc=9, lo=None, cnt=None, csum=None) == mpdata.EINVAL and b"condition tracer" in err()
        assert call(lo=None, cnt=None, csum=None) == mpdata.EINVAL and b"lo and hi" in err()
        assert call(cnt=None, csum=None, ntr=9) == mpdata.EINVAL and b"cnt and csum" in err()
        assert call(cnt=None, ntr=9) == mpdata.EINVAL and b"tracer range" in err()
    dev = lambda plan=one, sl0=0, n=1, tc=0, lo=one, cnt=one: L.mpdata_plan_level_cond_device(plan, sl0, n, tc, lo, None, cnt, None, 0, 0)
    assert dev(plan=None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_cond(None, 0, 1, 0, one, None, one, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_cond_f32(None, 0, 1, 0, one, None, one, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert dev(sl0=sl0, n=n) == mpdata.EINVAL
    assert dev(n=0, tc=9, lo=None, cnt=None) == mpdata.EINVAL and b"n = 0" in err()     # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_level_cond.hip: no scratch memory, no vector
    and no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS, has no barrier and
    no inline assembly.  Kernels: the plan-layout one in its two forms (MASK, RE-READ), each for double and float2
    elements; the reference-layout one for double and float."""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_level_cond.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_level_cond_kernel", txt)) == 4
    assert len(re.findall(r"Function Name: \S*ref_level_cond_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 6 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_level_cond.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_level_cond\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_level_cond", mk)
    assert "mpdata_level_cond$(O)" in mk.split("OBJS :=")[1].split("\n")[0]
    assert "mpdata_level_cond.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
