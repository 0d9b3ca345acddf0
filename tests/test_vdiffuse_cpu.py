"""CPU tests of the implicit vertical diffusion with a per-cell diffusivity (include/mpdata_hip.h 3s): the numpy model of
tests/vdiffuse_model.py against what is not itself -- a scalar triple loop of the section's statements, the model of 3o
with the coefficients folded, the dense fp64 solve of numpy.linalg, the discrete maximum principle --, the identity and
its stated exception, what is never read, the plan model's rules, and the interface (header, ctypes, Fortran, Python
names, the argument checks that need no device, the compiler's resource report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import vdiffuse_model as DV
import vsolve_model as VM
from oracle import plan_model as PM
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_vdiffuse_device", "mpdata_plan_vdiffuse", "mpdata_plan_vdiffuse_f32", "mpdata_vdiffuse_device",
         "mpdata_vdiffuse_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-0.5, 0.5, sh).astype(dtype))


def rho_adz(n, nz, dtype, seed):
    rng = np.random.default_rng([seed, n, nz, 5])
    return tuple(np.asfortranarray(rng.uniform(0.5, 1.0, (n, nz - 1)).astype(dtype)) for _ in range(2))


def case(n, nx, nz, T, dtype, seed, **kw):
    f = field(n, nx, nz, T, dtype, seed)
    rho, adz = rho_adz(n, nz, dtype, seed)
    return f, rho, adz, DV.make_coeffs(n, nx, nz, dtype, seed, **kw)


def call(f, rho, adz, c):
    return DV.vdiffuse(f, rho, adz, c["tkh"], c["cz"], c["sb"], c["st"])


# ---- 1. the model against something that is not itself
def scalar_loops(f, rho, adz, tkh, cz, sb, st):
    """section 3s statement by statement on numpy scalars of f's dtype: instance, column, tracer, then k"""
    R = f.dtype.type
    F = f.reshape(f.shape + (1,)) if f.ndim == 3 else f
    n, nxp6, nzm, T = F.shape
    nx = nxp6 - 6
    out = np.array(F, order="F")
    for b in range(n):
        ir = [R(1) / (rho[b, k] * adz[b, k]) for k in range(nzm)]
        for i in range(1, nx + 1):
            e = [R(0)] * (nzm + 1)
            for k in range(1, nzm):
                s = tkh[b, i, k - 1] + tkh[b, i, k]
                e[k] = cz[b, k - 1] * s
            a = [e[k] * ir[k] for k in range(nzm)]
            c = [e[k + 1] * ir[k] for k in range(nzm)]
            di = [(R(1) + a[k]) + c[k] for k in range(nzm)]
            for t in range(T):
                r = [F[b, i + 2, k, t] for k in range(nzm)]
                if sb is not None:
                    r[0] = r[0] + sb[b, i - 1] * ir[0]
                if st is not None:
                    r[nzm - 1] = r[nzm - 1] - st[b, i - 1] * ir[nzm - 1]
                g, y = [None] * nzm, [None] * nzm
                p = R(1) / di[0]
                g[0], y[0] = c[0] * p, r[0] * p
                for k in range(1, nzm):
                    m = a[k] * g[k - 1]
                    d = di[k] - m
                    p = R(1) / d
                    g[k] = c[k] * p
                    q = a[k] * y[k - 1]
                    v = r[k] + q
                    y[k] = v * p
                x = y[nzm - 1]
                out[b, i + 2, nzm - 1, t] = x
                for k in range(nzm - 2, -1, -1):
                    m = g[k] * x
                    x = y[k] + m
                    out[b, i + 2, k, t] = x
    assert out.dtype == f.dtype
    return out.reshape(f.shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(2, 3, 8, 2), (2, 1, 2, 1), (1, 2, 3, 1)], ids=["nzm7", "nzm1", "nzm2"])
@pytest.mark.parametrize("fluxes", [(True, True), (True, False), (False, True), (False, False)], ids=["sb-st", "sb", "st", "none"])
def test_model_equals_the_scalar_loops(dtype, shape, fluxes):
    n, nx, nz, T = shape
    f, rho, adz, c = case(n, nx, nz, T, dtype, 3)
    if not fluxes[0]:
        c["sb"] = None
    if not fluxes[1]:
        c["st"] = None
    got = call(f, rho, adz, c)
    want = scalar_loops(f, rho, adz, c["tkh"], c["cz"], c["sb"], c["st"])
    assert got.dtype == np.dtype(dtype) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(got, f) == (nz == 2 and not any(fluxes))          # (one level without fluxes: the identity)
    assert np.array_equal(bits(got[:, :3]), bits(f[:, :3])) and np.array_equal(bits(got[:, nx + 3:]), bits(f[:, nx + 3:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_one_level(dtype):
    """nzm = 1: e(0) = e(1) = +0, so a = c = +0, di = 1, p = 1: x = (f + sb ir) - st ir, the sb statement first"""
    n, nx = 3, 4
    f, rho, adz, c = case(n, nx, 2, 1, dtype, 4)
    R = np.dtype(dtype).type
    ir = R(1) / (rho * adz)
    want = np.array(f)
    want[:, 3:nx + 3, 0] = (f[:, 3:nx + 3, 0] + c["sb"] * ir) - c["st"] * ir
    nan = dict(c, tkh=np.full_like(c["tkh"], np.nan), cz=np.full_like(c["cz"], np.nan))    # neither is read at all
    assert np.array_equal(bits(call(f, rho, adz, nan)), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_identity_and_its_exception(dtype):
    """tkh = 0, or cz = 0, with NULL sb, st keeps every bit on inputs without -0.0; the stated exception: a = +0, so
    q = a * y(k-1) is +0.0 for a positive y(k-1) and v = -0.0 + +0.0 = +0.0"""
    n, nx, nz = 3, 4, 9
    f, rho, adz, c = case(n, nx, nz, 2, dtype, 5, fluxes=False)
    f[0, 4, 2] = 0.0
    assert not np.any(np.signbit(f) & (f == 0))
    zt, zc = np.zeros_like(c["tkh"]), np.zeros_like(c["cz"])
    assert np.array_equal(bits(DV.vdiffuse(f, rho, adz, zt, c["cz"])), bits(f))
    assert np.array_equal(bits(DV.vdiffuse(f, rho, adz, c["tkh"], zc)), bits(f))
    z = np.zeros((1, 7, 3), dtype, order="F")
    z[0, 3] = (1.0, -0.0, -0.0)
    x = DV.vdiffuse(z, rho[:1, :3], adz[:1, :3], zt[:1, :3, :3], c["cz"][:1, :3])
    # forward: level 2 is -0.0 + (+0 * 1.0) = +0.0; level 3 keeps -0.0 through it (+0 * +0.0 = +0.0 ... -0.0 + +0.0 = +0.0)
    assert x[0, 3, 0] == 1.0 and not np.signbit(x[0, 3, 1]) and x[0, 3, 1] == 0 and x[0, 3, 2] == 0
    # a lone -0.0 at level 1 keeps its sign through the forward sweep (y(1) = r * p) and loses it to x = y + g * x(k+1)
    z[0, 3] = (-0.0, 1.0, 1.0)
    x = DV.vdiffuse(z, rho[:1, :3], adz[:1, :3], zt[:1, :3, :3], c["cz"][:1, :3])
    assert x[0, 3, 0] == 0 and not np.signbit(x[0, 3, 0]) and x[0, 3, 1] == 1.0
    # ... and nzm = 1 keeps even that
    z1 = np.full((1, 7, 1), -0.0, dtype, order="F")
    assert np.array_equal(bits(DV.vdiffuse(z1, rho[:1, :1], adz[:1, :1], zt[:1, :3, :1], zc[:1, :1])), bits(z1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_a_column_without_diffusivity_keeps_its_bits_beside_one_with(dtype):
    n, nx, nz = 2, 5, 12
    f, rho, adz, c = case(n, nx, nz, 2, dtype, 6, fluxes=False)
    c["tkh"][:] = np.maximum(c["tkh"], np.dtype(dtype).type(0.125))
    c["tkh"][:, 3] = 0.0                                    # column 3 of 0 .. nx+1: interior column 3, array index 5 of f
    assert not np.any(np.signbit(f) & (f == 0))
    x = call(f, rho, adz, c)
    assert np.array_equal(bits(x[:, 5]), bits(f[:, 5]))
    for i in (1, 2, 4, 5):
        assert not np.array_equal(x[:, i + 2], f[:, i + 2]), i


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [2, 3, 9, 28])
def test_x_uniform_tkh_is_vsolve_with_the_signs_folded(dtype, nz):
    """tkh independent of i: the model of 3o with lo = -a, di, up = -c, bit for bit"""
    n, nx, T = 3, 4, 2
    f, rho, adz, c = case(n, nx, nz, T, dtype, 7, fluxes=False, x_uniform=True)
    assert (c["tkh"] == c["tkh"][:, 1:2]).all()
    _, a, cc, di = DV.coefficients(rho, adz, c["tkh"], c["cz"])
    assert (a == a[:, :1]).all() and (cc == cc[:, :1]).all()
    lo, d, up = (np.asfortranarray(v[:, 0]) for v in (-a, di, -cc))
    assert np.array_equal(bits(call(f, rho, adz, c)), bits(VM.vsolve(f, lo, d, up)))
    if nz > 2:
        assert (lo < 0).any() and not np.array_equal(call(f, rho, adz, c), f)


def test_halo_columns_of_tkh_and_the_top_of_cz_are_not_read():
    n, nx, nz = 2, 3, 7
    f, rho, adz, c = case(n, nx, nz, 1, np.float64, 8)
    want = call(f, rho, adz, c)
    t2, z2 = np.array(c["tkh"], order="F"), np.array(c["cz"], order="F")
    t2[:, 0], t2[:, -1], z2[:, -1] = np.nan, np.nan, np.nan
    assert np.array_equal(bits(call(f, rho, adz, dict(c, tkh=t2, cz=z2))), bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_zero_fluxes_equal_the_null_form_up_to_the_sign_of_zero(dtype):
    """sb, st given as +0 arrays: r(1) = f + (+0 * ir) = f + +0.0, which is f except that -0.0 becomes +0.0"""
    n, nx, nz = 2, 3, 7
    f, rho, adz, c = case(n, nx, nz, 2, dtype, 9, fluxes=False)
    zero = np.zeros((n, nx), dtype, order="F")
    null = call(f, rho, adz, c)
    assert np.array_equal(bits(call(f, rho, adz, dict(c, sb=zero, st=zero))), bits(null))
    # the sign of zero, on one level (above it the backward sweep's x = y + g x(k+1) decides): f(i,1) = -0.0
    g, rho1, adz1, c1 = case(n, nx, 2, 2, dtype, 9, fluxes=False)
    g[:, 3:nx + 3] = -0.0
    a, b = call(g, rho1, adz1, c1), call(g, rho1, adz1, dict(c1, sb=zero, st=zero))
    assert np.all(np.signbit(a[:, 3:nx + 3])) and not np.any(np.signbit(b[:, 3:nx + 3])) and np.array_equal(a, b)


ACC_NZM = (1, 2, 27, 64, 237)
ACC_SEEDS = 20
# measured with the seeds below, in units of u * max|r| (u = half the spacing at 1): the worst over ACC_NZM and the seeds
MEASURED = {np.float64: 6.03, np.float32: 15.27}
BOUND = {k: 4 * v for k, v in MEASURED.items()}


def accuracy_inputs(n, nx, nzm, dtype, seed, fluxes):
    """tkh uniform in [0, 1) with a third of the cells zero, cz = s * uniform [0, 1.8) with s = 1 for the first instance and
    10^-uniform[0, 3) for the others, rho and adz in [0.5, 1): the off-diagonals cz (tkh + tkh') ir span 0 to about 10 (below 14.4; the
    largest drawn is printed)"""
    f, rho, adz, c = case(n, nx, nzm + 1, 1, dtype, 40 + seed, fluxes=fluxes)
    rng = np.random.default_rng([90, seed, nzm])
    scale = 10.0 ** -rng.uniform(0.0, 3.0, (n, 1))
    scale[0] = 1.0                                          # (the first instance takes the full range)
    c["cz"] = np.asfortranarray((rng.uniform(0.0, 1.8, (n, nzm)) * scale).astype(dtype))
    return f, rho, adz, c


def dense(f, rho, adz, c, b, i):
    """(A, r) of instance b, interior column i in float64 from the same inputs"""
    nzm = rho.shape[1]
    ir = 1.0 / (rho[b].astype(np.float64) * adz[b].astype(np.float64))
    t = c["tkh"][b, i].astype(np.float64)
    e = np.zeros(nzm + 1)
    e[1:nzm] = c["cz"][b, :nzm - 1].astype(np.float64) * (t[:-1] + t[1:])
    a, cc = e[:-1] * ir, e[1:] * ir
    A = np.diag(1.0 + a + cc) - np.diag(a[1:], -1) - np.diag(cc[:-1], 1)
    r = f[b, i + 2].astype(np.float64)
    if c["sb"] is not None:
        r[0] += float(c["sb"][b, i - 1]) * ir[0]
    if c["st"] is not None:
        r[nzm - 1] -= float(c["st"][b, i - 1]) * ir[nzm - 1]
    return A, r


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_against_the_dense_fp64_solve_and_the_maximum_principle(dtype):
    """the model against numpy.linalg.solve on float64 copies of the same inputs (the matrix formed in float64 from tkh,
    cz, rho, adz), in units of u * max|r|, over nzm = 1, 2, 27, 64, 237 and 20 seeds, off-diagonals from 0 to 9.82.  The
    yardstick is the dense fp64 solve, not the code under test.  Measured: worst 6.028 (fp64) and 15.270 (fp32: there the
    roundings of s, e, a, c, di enter as well, which the float64 matrix does not share); the bound is 4 x that, 24.12 and
    61.08 -- the factor is the margin for other seeds.  On the same inputs without sb, st: every x(i,.) lies within
    [min f(i,.), max f(i,.)] widened by the same bound * u * max|f(i,.)| -- the matrix has row sums 1 and non-positive
    off-diagonals, so in exact arithmetic the maximum principle holds exactly (measured: beyond by 0.000 in both)."""
    u = float(np.finfo(dtype).eps) / 2
    worst, off, beyond = 0.0, 0.0, 0.0
    for nzm in ACC_NZM:
        for seed in range(ACC_SEEDS):
            n, nx = 2, 2
            f, rho, adz, c = accuracy_inputs(n, nx, nzm, dtype, seed, True)
            x = call(f, rho, adz, c)
            for b in range(n):
                for i in range(1, nx + 1):
                    A, r = dense(f, rho, adz, c, b, i)
                    ref = np.linalg.solve(A, r)
                    worst = max(worst, float(np.max(np.abs(x[b, i + 2].astype(np.float64) - ref))) / (u * float(np.max(np.abs(r)))))
                    off = max(off, float(-A.min()))
            # the maximum principle, without boundary fluxes
            c0 = dict(c, sb=None, st=None)
            x = call(f, rho, adz, c0).astype(np.float64)[:, 3:nx + 3]
            fi = f.astype(np.float64)[:, 3:nx + 3]
            lo, hi, mag = fi.min(axis=2), fi.max(axis=2), np.abs(fi).max(axis=2)
            over = np.maximum(x.max(axis=2) - hi, lo - x.min(axis=2)) / (u * mag)
            beyond = max(beyond, float(over.max()))
    print(f"vdiffuse against the dense fp64 solve, {np.dtype(dtype).name}: worst {worst:.3f} u max|r| (bound {BOUND[dtype]}), "
          f"largest off-diagonal {off:.2f}, beyond [min f, max f] by {beyond:.3f} u max|f|")
    assert 8.0 < off <= 14.4
    assert worst <= BOUND[dtype]
    assert beyond <= BOUND[dtype]


# ---- 2. the plan model: order of the checks, the block, the interior-only and the periodic rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = DV.PlanModelVdiffuse(oracle, *shape, T, dtype)
    return m, DV.make_plan_inputs(oracle, shape, T, dtype, 100)


def _args(c):
    return c["tkh"], c["cz"], c["sb"], c["st"]


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    c = _args(DV.make_coeffs(5, 8, 6, np.float64, 6))
    assert m.vdiffuse(*c) == PM.ESTATE                                     # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.vdiffuse(*c, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.vdiffuse(*c, first=1, ntr=2) == PM.EINVAL and m.vdiffuse(*c, first=-1, ntr=1) == PM.EINVAL
    assert m.vdiffuse(*c, first=0, ntr=0) == PM.EINVAL
    for i in range(2):
        a = list(c)
        a[i] = None
        assert m.vdiffuse(*a) == PM.EINVAL
        assert m.vdiffuse(*a, eb=4) == PM.EINVAL                           # the NULL comes before the precision
        m.windowed = True
        assert m.vdiffuse(*a) == PM.EINVAL                                 # ... and before the windows
        m.windowed = False
    assert m.vdiffuse(*c, eb=4) == PM.ESTATE                               # a host form of the other precision
    m.windowed = True
    assert m.vdiffuse(*c) == PM.EUNSUPPORTED and m.vdiffuse(*c, eb=4) == PM.EUNSUPPORTED     # the windows before the state
    assert m.vdiffuse(*c, first=0, ntr=3) == PM.EINVAL
    m.windowed = False
    m.multi = True
    assert m.vdiffuse(*c) == PM.EUNSUPPORTED and m.vdiffuse(*c, sl0=0, n=0) == PM.EINVAL
    assert m.vdiffuse(None, None) == PM.EUNSUPPORTED                       # the handle comes before the NULL
    m.multi = False
    for k, v in keep.items():
        assert np.array_equal(bits(m.a[k]), bits(v)), k
    assert m.vdiffuse(*c) is None and not np.array_equal(m.a["f"], keep["f"])
    assert np.array_equal(bits(m.a["f"][:, :3]), bits(keep["f"][:, :3]))                # halo columns keep every bit
    assert np.array_equal(bits(m.a["f"][:, 11:]), bits(keep["f"][:, 11:]))
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(bits(m.a[k]), bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_vdiffuse_is_export_change_import(oracle, boundary):
    """the call on a block and a tracer = export of the block, the solve with the block's rho and adz, import; on a
    PERIODIC model the halos of the next read-back are wrapped copies of the NEW interior"""
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    c = _args(DV.make_coeffs(3, 8, 6, np.float64, 7))
    assert a.vdiffuse(*c, sl0=1, n=3, first=1, ntr=1) is None
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new = DV.vdiffuse(exp[..., 0], inp["rho"][1:4], inp["adz"][1:4], *c)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k
    if boundary == PM.PERIODIC:
        e = ea["f"]
        assert np.array_equal(bits(e), bits(PM.wrap(np.array(e, order="F"))))
        assert np.array_equal(bits(e[1:4, 3:11, :, 1]), bits(new[:, 3:11]))            # ... of the new interior
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(bits(ea[k]), bits(eb[k])), k


# ---- 3. the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.vdiffuse) and callable(mpdata.Plan.vdiffuse) and callable(mpdata.Plan.vdiffuse_host)
    assert "vdiffuse" in mpdata.__all__ and "vdiffuse_shapes" in mpdata.__all__
    assert mpdata.vdiffuse_shapes(5, 4, 8) == {"tkh": (7, 6, 5), "cz": (7, 5), "sb": (4, 5), "st": (4, 5)}


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert hdr.index("---- 3r.") < hdr.index("---- 3s.") < hdr.index("---- 4.")
    sec = hdr.split("---- 3s.")[1].split("---- 4.")[0]
    for word in ("tkh", "cz", "sb", "st", "ir", "pivoting", "backward Euler", "diagonally dominant"):
        assert re.search(r"\b" + word + r"\b", sec, re.I), word
    assert "-0.0" in sec and "MPDATA_EUNSUPPORTED" in sec and "windowed" in sec.lower() and "zflux" in sec
    assert "bit for bit" in sec and "lo = -a" in sec and "up = -c" in sec
    assert "EXACT and FAST" in sec
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_plan_vdiffuse_device")] == \
        ["plan", "sl0", "n", "tkh", "cz", "sb", "st", "first_tracer", "ntracers"]
    assert [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, "mpdata_vdiffuse_device")] == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "rho", "adz", "tkh", "cz", "sb", "st", "stream"]


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
    m = re.search(r"integer\(c_int\) function mpdata_plan_vdiffuse_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_vdiffuse_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_vdiffuse_device")
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
    assert re.search(r"public ::.*\bmpdata_plan_vdiffuse_device_c\b", f90)
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "vdiffuse_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    ptrs = [one] * 7           # f, rho, adz, tkh, cz, sb, st
    for fn in (L.mpdata_vdiffuse_device, L.mpdata_vdiffuse_f32_device):
        assert fn(4, 0, 6, 1, 0, 4, *ptrs, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, *ptrs, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 4, *ptrs, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, *ptrs, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, *ptrs, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
        for i, nm in enumerate(("f", "rho", "adz", "tkh", "cz")):
            args = list(ptrs)
            args[i] = None
            assert fn(4, 5, 6, 1, 0, 4, *args, None) == mpdata.EINVAL, nm
            assert b"null " + nm.encode() in L.mpdata_last_error()
        none = [None] * 7
        assert fn(4, 5, 1, 1, 0, 4, *none, None) == mpdata.EINVAL and b"nz=1" in L.mpdata_last_error()      # sizes first
        assert fn(4, 5, 6, 1, 2, 3, *none, None) == mpdata.EINVAL and b"outside" in L.mpdata_last_error()   # then the block
        assert fn(4, 5, 6, 1, 0, 4, one, None, one, None, None, None, None, None) == mpdata.EINVAL
        assert b"null rho" in L.mpdata_last_error()                                                         # then f, rho, adz
        assert fn(4, 5, 6, 1, 0, 4, one, one, one, one, None, None, None, None) == mpdata.EINVAL
        assert b"null cz" in L.mpdata_last_error()                                                          # then tkh, cz
    assert L.mpdata_plan_vdiffuse_device(None, 0, 1, one, one, None, None, 0, 1) == mpdata.EINVAL
    assert b"null plan" in L.mpdata_last_error() and b"mpdata_plan_vdiffuse_device" in L.mpdata_last_error()
    assert L.mpdata_plan_vdiffuse(None, 0, 1, one, one, None, None) == mpdata.EINVAL
    assert L.mpdata_plan_vdiffuse_f32(None, 0, 1, one, one, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_vdiffuse_device(one, sl0, n, one, one, None, None, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_vdiffuse_device(one, 0, 0, None, None, None, None, 0, 1) == mpdata.EINVAL
    assert b"null tkh" not in L.mpdata_last_error()                                 # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_vdiffuse.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel; the LDS of the plan-layout kernel is dynamic, its budget ONE constant
    of the file, within what the file's head states and within a CU's 160 KiB, and the launch refuses a geometry beyond it"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_vdiffuse.usage.txt")
    assert os.path.exists(rep), "no resource-usage report: the library is built by __graft_entry__.build()"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_vdiffuse_kernel", txt)) == 2     # f64 and f32
    assert len(re.findall(r"Function Name: \S*vd_ir_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_vdiffuse_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 6 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    src = open(os.path.join(csrc, "mpdata_vdiffuse.hip")).read()
    walk = open(os.path.join(csrc, "mpdata_wm_walk.h")).read()
    m = re.findall(r"constexpr int VD_LDS_ELEMS = ([^;]+);", src)                          # (the one statement of the limit)
    assert len(m) == 1
    elems = int(re.search(r"constexpr int LDS_ELEMS = (\d+);", walk).group(1)) if m[0].strip() == "LDS_ELEMS" else int(m[0])
    stated = re.search(r"constexpr int VD_LDS_ELEMS = [^;]+;\s*//\s*(\d+) KiB", src)
    assert stated and elems * 8 <= int(stated.group(1)) * 1024 <= 160 * 1024
    assert "col_groups_batched(j, b.sel, wg, VD_LDS_ELEMS / 2," in src and "g->lds_e <= budget" in walk
    assert "cg.lds_e > VD_LDS_ELEMS" in src                                                # the launch refuses more
    mk = open(os.path.join(csrc, "Makefile")).read()
    rule = re.search(r"mpdata_vdiffuse\$\(O\):.*\n\t(.*)", mk)
    assert rule and "-ffp-contract=off" in rule.group(1) and "CC_USAGE" in rule.group(1)
