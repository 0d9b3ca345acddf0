"""CPU tests of the saturation adjustment (include/mpdata_hip.h 3y): the numpy model of tests/satadj_model.py against a
scalar triple loop and against what the definition implies -- rows with pres == 0, the inputs that are only read, a dry
field, the ice curve that is never read without ICE, a cell that stops on its own d, the merge property of level windows
--, the plan model's rules, and the interface (header and struct layout against ctypes, Fortran against the header, Python
names, the argument checks that need no device, the compiler's resource report).  No test here needs a GPU.

Every test that calls the model asserts the conditions of SA.check_conditions on its field."""
import ctypes
import os
import re

import numpy as np
import pytest

import satadj_model as SA
from oracle import plan_model as PM
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_satadj_device", "mpdata_plan_satadj", "mpdata_plan_satadj_f32", "mpdata_satadj_device", "mpdata_satadj_f32_device")
DTYPES = [np.float64, np.float32]
ORDER = (1, 3, 0, 4)      # th, tq, tn, tt


def field(n, nx, nz, dtype, seed, ice, gz_on, T=5):
    """f (n, nx+6, nzm, T) by the recipe, pres, gz or None, planted"""
    rng = np.random.default_rng([seed, 1])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1, T)).astype(dtype))
    pres, gz = SA.make_rows(n, nz, dtype, seed)
    gz = gz if gz_on else None
    f, planted = SA.fill_fields(f, ORDER[0], ORDER[1], pres, gz, SA.PAR, ice, seed)
    return f, pres, gz, planted


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the model against the definition
@pytest.mark.parametrize("tt_on", [True, False], ids=["tt", "nott"])
@pytest.mark.parametrize("gz_on", [True, False], ids=["gz", "nogz"])
@pytest.mark.parametrize("ice", [True, False], ids=["ice", "liq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_model_is_the_scalar_triple_loop(dtype, ice, gz_on, tt_on):
    f, pres, gz, planted = field(6, 9, 12, dtype, 3, ice, gz_on)
    th, tq, tn, tt = ORDER
    tt = tt if tt_on else -1
    for maxit in (10, 2, 1):
        par = SA.par_with(maxit=maxit)
        new, ncld, iters, info = SA.satadj(f, th, tq, tn, tt, pres, gz, par, ice, parts=True)
        SA.check_conditions(info, ice, maxit, planted)
        assert not ice or SA.edge_cells(f, th, pres, gz) >= 2
        new2, ncld2, iters2, its = SA.satadj_loops(f, th, tq, tn, tt, pres, gz, par, ice)
        assert same(new, new2) and same(ncld, ncld2) and same(iters, iters2)
        assert np.array_equal(its, np.where(info["on"], info["it"], 0))
        assert not same(new[..., tn], f[..., tn]) and (tt < 0 or not same(new[..., tt], f[..., tt]))
        assert its.max() == min(maxit, its.max()) and (maxit > 2 or its.max() == maxit)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_pres_zero_rows_and_inputs_keep_every_bit(dtype):
    f, pres, gz, planted = field(5, 4, 12, dtype, 4, True, True)
    th, tq, tn, tt = ORDER
    zero = pres == 0
    assert zero.any()
    f[:, 3:7, :, tn] = np.where(zero[:, None, :], -0.0, f[:, 3:7, :, tn])
    f[:, 3:7, :, tt] = np.where(zero[:, None, :], np.nan, f[:, 3:7, :, tt])
    f[:, 3:7, :, th] = np.where(zero[:, None, :], np.nan, f[:, 3:7, :, th])       # ... and are not read
    f[:, :3], f[:, 7:] = np.nan, -np.inf                                          # halo columns: neither read nor written
    new, ncld, iters, info = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, True, parts=True)
    SA.check_conditions(info, True, 10, planted)
    for t in (tn, tt):
        assert same(new[:, 3:7, :, t][np.broadcast_to(zero[:, None, :], (5, 4, 11))], f[:, 3:7, :, t][np.broadcast_to(zero[:, None, :], (5, 4, 11))])
    v = new[:, 3:7, :, tn][np.broadcast_to(zero[:, None, :], (5, 4, 11))]
    assert np.all(np.signbit(v) & (v == 0))
    assert not ncld[zero].any() and not iters[zero].any() and not np.signbit(ncld[zero]).any() and not np.signbit(iters[zero]).any()
    rest = [t for t in range(5) if t not in (tn, tt)]
    assert same(new[..., rest], f[..., rest]) and same(new[:, :3], f[:, :3]) and same(new[:, 7:], f[:, 7:])
    assert np.isfinite(new[:, 3:7, :, tn][np.broadcast_to(~zero[:, None, :], (5, 4, 11))]).all()
    # tt absent: tracer 4 keeps every bit too
    new2 = SA.satadj(f, th, tq, tn, -1, pres, gz, SA.PAR, True)[0]
    assert same(new2[..., tt], f[..., tt]) and same(new2[..., tn], new[..., tn])


@pytest.mark.parametrize("ice", [True, False], ids=["ice", "liq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_dry_field_gives_no_condensate_and_T1(dtype, ice):
    f, pres, gz, _ = field(4, 5, 12, dtype, 5, ice, True)
    th, tq, tn, tt = ORDER
    f[:, 3:8, :, tq] = f[:, 3:8, :, tq] * dtype(0.5)          # q <= 0.8 qs(T1)
    new, ncld, iters, info = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, ice, parts=True)
    on = info["on"]
    assert not info["wet"].any() and not ncld.any() and not iters.any()
    qn = new[:, 3:8, :, tn][on]
    assert not qn.any() and not np.signbit(qn).any()
    assert same(new[:, 3:8, :, tt][on], (f[:, 3:8, :, th] - gz[:, None, :])[on])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_without_ice_the_ice_numbers_are_never_read(dtype):
    f, pres, gz, planted = field(4, 5, 12, dtype, 6, False, True)
    th, tq, tn, tt = ORDER
    nan9 = [np.nan] * 9
    a = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, False, parts=True)
    SA.check_conditions(a[3], False, 10, planted)
    b = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.par_with(esi=nan9, desi=nan9, ls=np.nan, tmin=np.nan, tmax=np.nan), False)
    c = SA.satadj_loops(f, th, tq, tn, tt, pres, gz, SA.par_with(esi=nan9, desi=nan9, ls=np.nan, tmin=np.nan, tmax=np.nan), False)
    for x, y, z in zip(a[:3], b, c[:3]):
        assert same(x, y) and same(x, z)
    # ... and with ICE they are: another result
    assert not same(SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, True)[0], a[0])


@pytest.mark.parametrize("ice", [True, False], ids=["ice", "liq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_cell_stops_on_its_own_d(dtype, ice):
    """a cell alone in its field takes as many steps as among its neighbours, and ends on the same bits"""
    f, pres, gz, planted = field(3, 6, 12, dtype, 7, ice, True)
    th, tq, tn, tt = ORDER
    new, _, _, info = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, ice, parts=True)
    SA.check_conditions(info, ice, 10, planted)
    it = info["it"]
    assert len(np.unique(it[info["wet"]])) >= 3
    for steps in np.unique(it[info["wet"]]):
        b, i, k = [int(x[0]) for x in np.nonzero(info["wet"] & (it == steps))]
        one = np.asfortranarray(f[b:b + 1, i:i + 7, k:k + 1])            # the cell as column 1 of a field of its own (nx = 1)
        got, _, its1, _ = SA.satadj(one, th, tq, tn, tt, np.asfortranarray(pres[b:b + 1, k:k + 1]),
                                    np.asfortranarray(gz[b:b + 1, k:k + 1]), SA.PAR, ice, parts=True)
        assert its1[0, 0] == steps
        assert same(got[0, 3, 0, [tn, tt]], new[b, i + 3, k, [tn, tt]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [239, 300])
def test_windows_merge_to_the_tall_operator(mpdata, nz, dtype):
    """the operator on every level window as a problem of its own (with pres and gz of the tall levels), owned levels merged
    == the operator on the tall column, bit for bit; ncld and iters from each level's owner.  The geometry is the library's."""
    n, nx = 2, 3
    nzm = nz - 1
    f, pres, gz, planted = field(n, nx, nz, dtype, 21, True, True)
    th, tq, tn, tt = ORDER
    want, wn, wi, info = SA.satadj(f, th, tq, tn, tt, pres, gz, SA.PAR, True, parts=True)
    SA.check_conditions(info, True, 10, planted)
    W = mpdata.level_window(nz, 0)[0]
    assert W > 1
    got, gn, gi = np.array(f, order="F"), np.full_like(wn, np.nan), np.full_like(wi, np.nan)
    owned = np.zeros(nzm, int)
    for h in range(W):
        _, k0, nz_w, own0, own1 = mpdata.level_window(nz, h)
        lev = slice(k0, k0 + nz_w - 1)
        new, c, i = SA.satadj(np.asfortranarray(f[:, :, lev]), th, tq, tn, tt, np.asfortranarray(pres[:, lev]),
                              np.asfortranarray(gz[:, lev]), SA.PAR, True)
        own = slice(own0 - 1, own1)                      # tall, 0-based
        loc = slice(own0 - 1 - k0, own1 - k0)            # in the window
        got[:, :, own], gn[:, own], gi[:, own] = new[:, :, loc], c[:, loc], i[:, loc]
        owned[own] += 1
    assert np.all(owned == 1)                            # every tall level owned exactly once
    assert same(got, want) and same(gn, wn) and same(gi, wi)


# ---- the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, shape=(5, 8, 12)):
    import subside_model as UM
    m = SA.PlanModelSatadj(oracle, *shape, 5, dtype)
    inp = dict(UM.make_plan_inputs(oracle, shape, 5, dtype, 100))
    pres, gz = SA.make_rows(shape[0], shape[2], dtype, 8)
    inp["f"], planted = SA.fill_fields(inp["f"], ORDER[0], ORDER[1], pres, gz, SA.PAR, True, 8)
    return m, inp, pres, gz


def test_plan_model_errors_change_nothing(oracle):
    m, inp, pres, gz = _model(oracle)
    th, tq, tn, tt = ORDER
    call = lambda **kw: m.satadj(**{**dict(th=th, tq=tq, tn=tn, tt=tt, pres=pres, gz=gz, par=SA.PAR, mode=1), **kw})
    assert call() == PM.ESTATE                                                # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    p1 = np.asfortranarray(pres[:1])
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert call(sl0=sl0, n=n, pres=p1, gz=None) == PM.EINVAL, (sl0, n)
    for kw in (dict(th=-1), dict(th=5), dict(tq=5), dict(tn=-1), dict(tn=5), dict(tt=-2), dict(tt=5), dict(tq=th), dict(tn=th), dict(tn=tq),
               dict(tt=th), dict(tt=tq), dict(tt=tn), dict(pres=None), dict(par=None), dict(par=SA.par_with(maxit=0)),
               dict(par=SA.par_with(maxit=33)), dict(par=SA.par_with(tol=-1.0)), dict(par=SA.par_with(tol=np.nan)),
               dict(par=SA.par_with(tmin=280.0)), dict(par=SA.par_with(tmax=np.nan)), dict(mode=2), dict(mode=3)):
        assert call(**kw) == PM.EINVAL, kw
    assert call(eb=4) == PM.ESTATE                                            # a host form of the other precision
    assert call(eb=4, mode=2) == PM.EINVAL                                    # its arguments come first
    m.multi = True
    assert call() == PM.EUNSUPPORTED and call(sl0=0, n=0) == PM.EINVAL and call(tn=tq) == PM.EUNSUPPORTED
    m.multi = False
    for k, v in keep.items():
        assert same(m.a[k], v), k
    assert not isinstance(call(par=SA.par_with(tmin=280.0), mode=0), int)     # (without ICE the ramp is not looked at)
    ncld, iters = call()
    assert ncld.shape == (5, 11) and iters.shape == (5, 11) and not same(m.a["f"], keep["f"])
    assert same(m.a["f"][:, :3], keep["f"][:, :3]) and same(m.a["f"][:, 11:], keep["f"][:, 11:])      # halo columns keep every bit
    assert same(m.a["f"][..., [th, tq, 2]], keep["f"][..., [th, tq, 2]])
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert same(m.a[k], keep[k]), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_satadj_is_export_change_import(oracle, boundary):
    """the call on a block = export of the block, the operator, import; on a PERIODIC model the halos of the next read-back
    are wrapped copies of the NEW interior of tn and tt"""
    a, inp, pres, gz = _model(oracle)
    b = _model(oracle)[0]
    th, tq, tn, tt = ORDER
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None
    pb, gb = np.asfortranarray(pres[1:4]), np.asfortranarray(gz[1:4])
    ncld, iters = a.satadj(th, tq, tn, tt, pb, gb, SA.PAR, 1, sl0=1, n=3)
    exp = b.export_block(1, 3, ("f",), 0, 5)["f"]
    new, c2, i2 = SA.satadj(exp, th, tq, tn, tt, pb, gb, SA.PAR, True)
    assert b.import_block(1, 3, {"f": new}, 0, 5) is None
    assert same(ncld, c2) and same(iters, i2)
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert same(ea[k], eb[k]), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert same(e, PM.wrap(np.array(e, order="F")))
        assert same(e[1:4, 3:11, :, tn], new[:, 3:11, :, tn])                 # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert same(ea[k], eb[k]), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.satadj) and callable(mpdata.Plan.satadj) and callable(mpdata.Plan.satadj_host)
    for nm in ("satadj", "satadj_shapes", "SatadjParams", "SATADJ_ICE"):
        assert nm in mpdata.__all__, nm
    assert mpdata.SATADJ_ICE == 1
    assert mpdata.satadj_shapes(5, 3, 8) == {k: (7, 5) for k in ("pres", "gz", "ncld", "iters")}
    p = mpdata.SatadjParams(**SA.PAR)
    assert list(p.esw) == SA.PAR["esw"] and list(p.desi) == SA.PAR["desi"] and p.maxit == 10 and p.tmax == 273.16
    with pytest.raises(mpdata.MpdataError):
        mpdata.SatadjParams(esw=[1.0] * 8)
    with pytest.raises(mpdata.MpdataError):
        mpdata.SatadjParams(nothing=1)


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def _header():
    return open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()


def test_header_section():
    hdr = _header()
    assert "---- 3y." in hdr
    sec = hdr.split("---- 3y.")[1].split("---- 4.")[0]
    for word in ("pres", "gz", "ncld", "iters", "esw", "desi", "an", "bn", "lf", "fff", "dfff", "maxit", "tol", "xmin"):
        assert re.search(r"\b" + word + r"\b", sec), word
    assert "windowed plans" in sec.lower() and "are supported" in sec and "owned levels only" in sec
    assert "rounded once" in sec and "correctly rounded IEEE division" in sec and "never fmax / fmin" in sec
    assert "ITS OWN d" in sec and "pres(b,k) == 0" in sec and "#define MPDATA_SATADJ_ICE 1" in sec
    assert hdr.index("---- 3x.") < hdr.index("---- 3y.") < hdr.index("---- 4.")
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", sec), n


def _struct_fields(hdr):
    """[(name, count)] of struct mpdata_satadj_params, in order, with the C type of each"""
    body = re.search(r"typedef struct mpdata_satadj_params \{(.*?)\} mpdata_satadj_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), int(m.group(2) or 1), ctype))
    return out


def test_struct_layout_ctypes_and_fortran_agree_with_the_header(mpdata):
    fields = _struct_fields(_header())
    assert [f[0] for f in fields] == ["esw", "desw", "esi", "desi", "t0", "xmin", "eps", "lv", "ls", "tmin", "tmax", "tol", "maxit"]
    py = mpdata.SatadjParams._fields_
    assert [n for n, _ in py] == [f[0] for f in fields]
    for (name, count, ctype), (_, t) in zip(fields, py):
        want = {"double": ctypes.c_double, "int": ctypes.c_int}[ctype]
        assert t is (want * count if count > 1 else want) or (count > 1 and t._type_ is want and t._length_ == count), name
    assert ctypes.sizeof(mpdata.SatadjParams) == 36 * 8 + 8 * 8 + 8 and mpdata.SatadjParams.maxit.offset == 44 * 8
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    body = re.search(r"type, bind\(C\) :: mpdata_satadj_params\n(.*?)end type", f90, re.S).group(1)
    got = []
    for line in body.splitlines():
        line = line.split("!")[0]
        m = re.match(r"\s*(real\(c_double\)|integer\(c_int\)) :: (.*)", line)
        if m:
            for nm in m.group(2).split(","):
                d = re.match(r"\s*(\w+)(?:\((\d+)\))?\s*$", nm)
                got.append((d.group(1), int(d.group(2) or 1), {"real(c_double)": "double", "integer(c_int)": "int"}[m.group(1)]))
    assert got == fields
    assert re.search(r"public :: mpdata_satadj_params\b", f90) and re.search(r"MPDATA_SATADJ_ICE = 1\b", f90)


def test_library_exports_and_ctypes_agree_with_the_header(mpdata):
    hdr = _header()
    L = mpdata.lib()
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            if a is ctypes.c_void_p or a is ctypes.POINTER(mpdata.SatadjParams):
                assert "*" in p and (("mpdata_satadj_params" in p) == (a is not ctypes.c_void_p)), (n, p, a)
            else:
                k = {ctypes.c_int64: "int64_t", ctypes.c_int: "int"}[a]
                assert p.startswith(k + " ") and "*" not in p, (n, p, a)
    names = lambda n: [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)]
    tail = ["th", "tq", "tn", "tt", "pres", "gz", "par", "mode", "ncld", "iters"]
    assert names("mpdata_plan_satadj_device") == names("mpdata_plan_satadj") == names("mpdata_plan_satadj_f32") == ["plan", "sl0", "n"] + tail
    assert names("mpdata_satadj_device") == names("mpdata_satadj_f32_device") == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f"] + tail + ["stream"]


def test_fortran_interfaces_agree_with_the_header():
    """the five interfaces, each bound by the literal name, public, the dummy arguments in the header's order, each of the
    header's kind and passed by value"""
    hdr = _header()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    for cname in NAMES:
        fname = cname + "_c"
        m = re.search(r"integer\(c_int\) function " + fname + r"\(([^)]*)\)\s*&?\s*bind\(C, name=\"" + cname + r"\"\)(.*?)end function",
                      f90, re.S)
        assert m, cname
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        params = _c_params(hdr, cname)
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
            assert decl.get(a) == want, (cname, a, p, decl.get(a))
        assert re.search(r"public ::.*\b" + fname + r"\b", f90), fname
    # in the second interface block, behind 3x's bindings
    assert f90.index("mpdata_nonneg_f32_device_c(ncrms") < f90.index("mpdata_plan_satadj_device_c(plan")
    assert f90.count("\n  interface\n") == 2 and f90.rindex("\n  interface\n") < f90.index("mpdata_plan_satadj_device_c(plan")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "satadj_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\bsatadj\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    err = L.mpdata_last_error
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    P = lambda **kw: ctypes.byref(mpdata.SatadjParams(**SA.par_with(**kw)))
    par = P()
    for fn in (L.mpdata_satadj_device, L.mpdata_satadj_f32_device):
        arr = lambda ncrms=4, nx=5, nz=6, nt=4, sl0=0, n=4, f=one, th=0, tq=1, tn=2, tt=3, pres=one, par=par, mode=0: \
            fn(ncrms, nx, nz, nt, sl0, n, f, th, tq, tn, tt, pres, None, par, mode, None, None, None)
        assert arr(nx=0) == mpdata.EINVAL and arr(ncrms=0) == mpdata.EINVAL and arr(nt=0) == mpdata.EINVAL
        assert arr(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert arr(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert arr(f=None) == mpdata.EINVAL and b"null f" in err()
        for kw in (dict(th=-1), dict(th=4), dict(tq=-1), dict(tq=4), dict(tn=-1), dict(tn=4)):
            assert arr(**kw) == mpdata.EINVAL and b"outside the" in err(), kw
        for tt in (-2, 4):
            assert arr(tt=tt) == mpdata.EINVAL and b"tt =" in err()
        for kw in (dict(tq=0), dict(tn=0), dict(tn=1), dict(tt=0), dict(tt=1), dict(tt=2)):
            assert arr(**kw) == mpdata.EINVAL and b"not distinct" in err(), kw
        assert arr(pres=None) == mpdata.EINVAL and b"null pres" in err()
        assert arr(par=None) == mpdata.EINVAL and b"null par" in err()
        for maxit in (0, -3, 33):
            assert arr(par=P(maxit=maxit)) == mpdata.EINVAL and b"maxit" in err()
        for tol in (-0.5, float("nan")):
            assert arr(par=P(tol=tol)) == mpdata.EINVAL and b"tol" in err()
        for tmin, tmax in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("nan"))):
            assert arr(par=P(tmin=tmin, tmax=tmax), mode=1) == mpdata.EINVAL and b"tmax" in err()
        for mode in (2, 3, -1, 256):
            assert arr(mode=mode) == mpdata.EINVAL and b"mode" in err()
        # the order
        assert arr(nz=1, sl0=2, n=3, f=None, th=9, pres=None, par=None, mode=2) == mpdata.EINVAL and b"nz=1" in err()
        assert arr(sl0=2, n=3, f=None, th=9, pres=None, par=None, mode=2) == mpdata.EINVAL and b"outside the arrays" in err()
        assert arr(f=None, th=9, pres=None, par=None, mode=2) == mpdata.EINVAL and b"null f" in err()
        assert arr(th=9, tt=9, tn=1, pres=None, par=None, mode=2) == mpdata.EINVAL and b"outside the" in err()
        assert arr(tt=9, tn=1, pres=None, par=None, mode=2) == mpdata.EINVAL and b"tt =" in err()
        assert arr(tn=1, pres=None, par=None, mode=2) == mpdata.EINVAL and b"not distinct" in err()
        assert arr(pres=None, par=None, mode=2) == mpdata.EINVAL and b"null pres" in err()
        assert arr(par=None, mode=2) == mpdata.EINVAL and b"null par" in err()
        assert arr(par=P(maxit=0, tol=-1.0, tmin=2.0, tmax=1.0), mode=3) == mpdata.EINVAL and b"maxit" in err()
        assert arr(par=P(tol=-1.0, tmin=2.0, tmax=1.0), mode=3) == mpdata.EINVAL and b"tol" in err()
        assert arr(par=P(tmin=2.0, tmax=1.0), mode=3) == mpdata.EINVAL and b"tmax" in err()
        assert arr(par=P(tmin=2.0, tmax=1.0), mode=2) == mpdata.EINVAL and b"mode" in err()
    for fn in (L.mpdata_plan_satadj_device, L.mpdata_plan_satadj, L.mpdata_plan_satadj_f32):
        assert fn(None, 0, 1, 0, 1, 2, 3, one, None, par, 0, None, None) == mpdata.EINVAL and b"null plan" in err()
        assert fn(None, 0, 1, 0, 0, 0, 0, None, None, None, 9, None, None) == mpdata.EINVAL and b"null plan" in err()
        for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
            assert fn(one, sl0, n, 0, 1, 2, 3, one, None, par, 0, None, None) == mpdata.EINVAL


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_satadj.hip: no scratch memory, no vector and
    no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS, has no barrier and no
    inline assembly"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_satadj.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    # the plan-layout kernel for ICE x tt x precision; the reference-layout kernel for ICE x precision
    assert len(re.findall(r"Function Name: \S*wm_satadj_kernel", txt)) == 8
    assert len(re.findall(r"Function Name: \S*ref_satadj_kernel", txt)) == 4
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 12 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_satadj.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "asm" not in code and "fmax" not in code and "fmin" not in code
    assert "__ballot" in code and "__shfl" not in code and "__builtin_amdgcn_ds" not in code and "dpp" not in code.lower()
    # the columns a lane iterates at a time: the one the header and the GPU tests name
    m = re.search(r"#define MPDATA_SATADJ_NC (\d+)", open(os.path.join(csrc, "mpdata_satadj.h")).read())
    assert m and int(m.group(1)) in (1, 2, 4, 8)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_satadj\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_satadj", mk)
    assert "mpdata_satadj$(O)" in mk.split("OBJS :=")[1].splitlines()[0] and "mpdata_satadj.h " in mk
    assert "mpdata_satadj.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
