"""CPU tests of the eddy diffusion (include/mpdata_hip.h 3l): the numpy model of tests/diffuse_model.py against the
properties the definition implies, the plan model's rules, and the interface (header, ctypes, Fortran, Python names, the
argument checks that need no device, the compiler's resource report).  No test here needs a GPU.

Rounding bounds.  u = eps / 2 of the dtype, fmax = max |f|, Fm = a bound of every flux: max(cx, cz) * 2 max(tkh) * 2 fmax
(and max |sb|, |st|), formed in float64 from the inputs alone.
  telescoping (rho * adz = 1, so ir = 1 and the multiply is exact): per cell the roundings are Fx(i) - Fx(i-1), Fz(k) -
    Fz(k-1), their sum and f - sum: four, each at most u times a magnitude <= A = fmax + 4 Fm; summed over nx cells that is
    4 nx u A.  Each entry of zflux is nx adds whose partial sums are at most nx Fm: nx^2 u Fm, two entries per level.
  maximum principle (ir <= 4): each of the four fluxes carries two roundings after the weight is formed (2 u Fm each), the
    two differences one (u 2 Fm each), the z part is multiplied by ir <= 4 (x 4, and one more rounding u 8 Fm), the sum one
    (u 10 Fm), the final subtraction one (u (fmax + 10 Fm)): (8 + 4 * 6 + 2 + 8 + 10 + 10) u Fm + u fmax <= 64 u (fmax + Fm).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import diffuse_model as DM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_diffuse_device", "mpdata_plan_diffuse", "mpdata_plan_diffuse_f32", "mpdata_diffuse_device",
         "mpdata_diffuse_f32_device")
DTYPES = [np.float64, np.float32]


def field(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng([seed, n, nx, nz, T])
    sh = (n, nx + 6, nz - 1) + ((T,) if T > 1 else ())
    return np.asfortranarray(rng.uniform(-1.0, 1.0, sh).astype(dtype))


def ones(n, nz, dtype):
    return np.ones((n, nz - 1), dtype, order="F")


# ---- the model against the definition's consequences
@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_field_keeps_every_bit(dtype):
    n, nx, nz = 3, 8, 6
    c = DM.make_coeffs(n, nx, nz, dtype, 1, fluxes=False)
    rng = np.random.default_rng(5)
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (n, nz - 1)).astype(dtype)) for _ in range(2))
    for value in (0.3, -7.25, 0.0, -0.0):
        f = np.full((n, nx + 6, nz - 1), value, dtype, order="F")
        new, zflux = DM.diffuse(f, rho, adz, **c)
        assert np.array_equal(DM.bits(new), DM.bits(f)), value
        assert not np.any(zflux) and not np.any(np.signbit(zflux))        # +0 throughout


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_zflux_telescopes(dtype, T):
    n, nx, nz = 5, 8, 6
    nzm = nz - 1
    f = field(n, nx, nz, T, dtype, 11)
    c = DM.make_coeffs(n, nx, nz, dtype, 2)
    new, zflux = DM.diffuse(f, ones(n, nz, dtype), ones(n, nz, dtype), **c)
    L = np.longdouble
    F = f.reshape((n, nx + 6, nzm, T)).astype(L)
    N = new.reshape((n, nx + 6, nzm, T)).astype(L)
    Z = zflux.reshape((n, nz, T)).astype(L)
    # the x-boundary fluxes Fx(0), Fx(nx) exactly as the definition rounds them
    tk, cx = c["tkh"], c["cx"][:, :, None]
    fr = f.reshape((n, nx + 6, nzm, T))
    fx0 = -((cx * (tk[:, 0] + tk[:, 1])[..., None]) * (fr[:, 3] - fr[:, 2]))
    fxn = -((cx * (tk[:, nx] + tk[:, nx + 1])[..., None]) * (fr[:, nx + 3] - fr[:, nx + 2]))
    assert fx0.dtype == dtype and fxn.dtype == dtype
    lhs = (N[:, 3:nx + 3] - F[:, 3:nx + 3]).sum(axis=1)
    rhs = Z[:, :-1] - Z[:, 1:] + fx0.astype(L) - fxn.astype(L)
    u = float(np.finfo(dtype).eps) / 2
    fmax = float(np.abs(f).max())
    Fm = max(float(max(c["cx"].max(), c["cz"].max())) * 2 * float(c["tkh"].max()) * 2 * fmax, float(np.abs(c["sb"]).max()),
             float(np.abs(c["st"]).max()))
    bound = u * (4 * nx * (fmax + 4 * Fm) + 2 * nx * nx * Fm)
    err = float(np.abs(lhs - rhs).max())
    print(f"telescoping {np.dtype(dtype).name} T={T}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(np.abs(lhs).max()) > 1e3 * bound        # (the sums are not zero: the test sees something)
    # the surface and top rows are the sums of sb and st alone
    s0 = np.zeros(n, dtype)
    s1 = np.zeros(n, dtype)
    for i in range(nx):
        s0, s1 = s0 + c["sb"][:, i], s1 + c["st"][:, i]
    for t in range(T):
        assert np.array_equal(Z[:, 0, t], s0.astype(L)) and np.array_equal(Z[:, nzm, t], s1.astype(L))
    # only the interior columns changed
    assert np.array_equal(DM.bits(new[:, :3]), DM.bits(f[:, :3])) and np.array_equal(DM.bits(new[:, nx + 3:]), DM.bits(f[:, nx + 3:]))
    assert not np.array_equal(new[:, 3:nx + 3], f[:, 3:nx + 3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_maximum_principle(dtype):
    n, nx, nz = 5, 8, 12
    nzm = nz - 1
    f = field(n, nx, nz, 1, dtype, 12)
    c = DM.make_coeffs(n, nx, nz, dtype, 3, fluxes=False)
    rng = np.random.default_rng(6)
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (n, nzm)).astype(dtype)) for _ in range(2))
    ir = 1.0 / (rho.astype(np.float64) * adz)
    tmax = float(c["tkh"].max())
    assert np.all(2 * c["cx"].astype(np.float64) * tmax * 2 + 2 * c["cz"].astype(np.float64) * tmax * 2 * ir <= 1.0)
    new, _ = DM.diffuse(f, rho, adz, **c)
    ctr = f[:, 3:nx + 3]
    lo = np.minimum(np.minimum(f[:, 2:nx + 2], f[:, 4:nx + 4]), ctr)
    hi = np.maximum(np.maximum(f[:, 2:nx + 2], f[:, 4:nx + 4]), ctr)
    lo[:, :, 1:] = np.minimum(lo[:, :, 1:], ctr[:, :, :-1]); hi[:, :, 1:] = np.maximum(hi[:, :, 1:], ctr[:, :, :-1])
    lo[:, :, :-1] = np.minimum(lo[:, :, :-1], ctr[:, :, 1:]); hi[:, :, :-1] = np.maximum(hi[:, :, :-1], ctr[:, :, 1:])
    u = float(np.finfo(dtype).eps) / 2
    fmax = float(np.abs(f).max())
    Fm = float(max(c["cx"].max(), c["cz"].max())) * 2 * tmax * 2 * fmax
    bound = 64 * u * (fmax + Fm)
    got = new[:, 3:nx + 3].astype(np.float64)
    over = float(max((got - hi).max(), (lo - got).max()))
    print(f"maximum principle {np.dtype(dtype).name}: largest excursion {over:.3e}, bound {bound:.3e}")
    assert over <= bound
    assert float(np.abs(got - ctr).max()) > 1e3 * bound         # (the field moved: the test sees something)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_wrong_vertical_neighbour_shows(dtype):
    """tkh of make_coeffs alternates by a factor 16 from level to level: taking tkh(k) or tkh(k-1) for tkh(k+1) moves f by
    far more than a rounding"""
    n, nx, nz = 3, 8, 6
    f = field(n, nx, nz, 1, dtype, 13)
    c = DM.make_coeffs(n, nx, nz, dtype, 4)
    new, _ = DM.diffuse(f, ones(n, nz, dtype), ones(n, nz, dtype), **c)
    bad = dict(c, tkh=np.asfortranarray(np.roll(c["tkh"], 1, axis=2)))
    new2, _ = DM.diffuse(f, ones(n, nz, dtype), ones(n, nz, dtype), **bad)
    assert float(np.abs(new - new2).max()) > 1e-3
    assert float(c["tkh"][:, :, 0].min()) > 4 * float(c["tkh"][:, :, 1].max())


def test_one_tracer_with_and_without_axis_and_tracers_share_tkh():
    n, nx, nz = 3, 3, 6
    f = field(n, nx, nz, 2, np.float64, 14)
    c = DM.make_coeffs(n, nx, nz, np.float64, 5)
    r = ones(n, nz, np.float64)
    new, zf = DM.diffuse(f, r, r, **c)
    for t in range(2):
        n1, z1 = DM.diffuse(np.asfortranarray(f[..., t]), r, r, **c)
        assert np.array_equal(DM.bits(n1), DM.bits(new[..., t])) and np.array_equal(DM.bits(z1), DM.bits(zf[..., t]))


# ---- the plan model: order of the checks, the block and the halo rule
def _model(oracle, dtype=np.float64, T=2, shape=(5, 8, 6)):
    m = DM.PlanModelDiffuse(oracle, *shape, T, dtype)
    return m, DM.make_plan_inputs(oracle, shape, T, dtype, 100)


def test_plan_model_errors_change_nothing(oracle):
    m, inp = _model(oracle)
    c = DM.make_coeffs(5, 8, 6, np.float64, 6)
    assert m.diffuse(**c) == PM.ESTATE                                   # never filled
    assert m.upload(inp) is None
    keep = {k: np.array(v) for k, v in m.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.diffuse(**c, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    assert m.diffuse(**c, first=1, ntr=2) == PM.EINVAL and m.diffuse(**c, first=-1, ntr=1) == PM.EINVAL
    assert m.diffuse(**c, first=0, ntr=0) == PM.EINVAL
    for k in ("tkh", "cx", "cz"):
        assert m.diffuse(**dict(c, **{k: None})) == PM.EINVAL
    assert m.diffuse(**c, eb=4) == PM.ESTATE                             # a host form of the other precision
    m.multi = True
    assert m.diffuse(**c) == PM.EUNSUPPORTED and m.diffuse(**c, sl0=0, n=0) == PM.EINVAL
    m.multi = False
    m.windowed = True
    assert m.diffuse(**c) == PM.EUNSUPPORTED and m.diffuse(**dict(c, tkh=None)) == PM.EINVAL
    m.windowed = False
    for k, v in keep.items():
        assert np.array_equal(DM.bits(m.a[k]), DM.bits(v)), k
    z = m.diffuse(**c)
    assert z.shape == (5, 6, 2) and not np.array_equal(m.a["f"], keep["f"])
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(DM.bits(m.a[k]), DM.bits(keep[k])), k


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_diffuse_is_export_change_import(oracle, boundary):
    a, inp = _model(oracle)
    b, _ = _model(oracle)
    for m in (a, b):
        assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None     # (halos stale)
    c = DM.make_coeffs(3, 8, 6, np.float64, 7)
    z = a.diffuse(**c, sl0=1, n=3, first=1, ntr=1)
    exp = b.export_block(1, 3, ("f",), 1, 1)["f"]
    new, z2 = DM.diffuse(exp[..., 0], inp["rho"][1:4], inp["adz"][1:4], **c)
    assert b.import_block(1, 3, {"f": new}, 1, 1) is None
    assert np.array_equal(DM.bits(z[..., 0]), DM.bits(z2))
    for m in (a, b):
        assert m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(DM.bits(ea[k]), DM.bits(eb[k])), k
    # outside the block and the tracer range nothing moved
    c0, _ = _model(oracle)
    assert c0.upload(inp) is None and c0.set_boundary(boundary) is None and c0.run() is None
    a2, _ = _model(oracle)
    assert a2.upload(inp) is None and a2.set_boundary(boundary) is None and a2.run() is None
    a2.diffuse(**c, sl0=1, n=3, first=1, ntr=1)
    fa, f0 = a2.export_device(("f",))["f"], c0.export_device(("f",))["f"]
    assert np.array_equal(DM.bits(fa[..., 0]), DM.bits(f0[..., 0]))
    assert np.array_equal(DM.bits(fa[[0, 4]]), DM.bits(f0[[0, 4]]))
    assert not np.array_equal(fa[1:4, ..., 1], f0[1:4, ..., 1])


# ---- the interface (files parsed: no device)
def test_shapes(mpdata):
    sh = mpdata.diffuse_shapes(5, 8, 6)
    assert sh == {"tkh": (5, 10, 5), "cx": (5, 5), "cz": (5, 5), "sb": (8, 5), "st": (8, 5), "zflux": (6, 5)}
    assert mpdata.diffuse_shapes(5, 8, 6, 3)["zflux"] == (3, 6, 5) and mpdata.diffuse_shapes(5, 8, 6, 1)["zflux"] == (1, 6, 5)
    # the reversed-axes views of the model's arrays
    c = DM.make_coeffs(5, 8, 6, np.float64, 8)
    for k in ("tkh", "cx", "cz", "sb", "st"):
        assert c[k].T.shape == sh[k], k
    assert callable(mpdata.diffuse) and callable(mpdata.Plan.diffuse) and callable(mpdata.Plan.diffuse_host)
    assert "diffuse" in mpdata.__all__ and "diffuse_shapes" in mpdata.__all__


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_ctypes_and_fortran_agree(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    assert "---- 3l." in hdr and "windowed" in hdr.split("---- 3l.")[1].split("---- 4.")[0].lower()
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)
        assert re.search(r'"' + n + r'"', f90), f"Fortran interface: {n}"
    # Fortran: the dummy arguments of each interface, in the header's order
    pairs = (("mpdata_plan_diffuse_device_c", "mpdata_plan_diffuse_device"), ("mpdata_plan_diffuse_c", "mpdata_plan_diffuse"),
             ("mpdata_diffuse_device_c", "mpdata_diffuse_device"))
    for fname, cname in pairs:
        m = re.search(r"integer\(c_int\) function " + fname + r"\(([^)]*)\)", f90)
        assert m, fname
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        cargs = [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, cname)]
        assert fargs == cargs, (fname, fargs, cargs)
        assert re.search(r"public ::.*\b" + fname + r"\b", f90), fname
    assert 'MPDATA_C_PLAN_DIFFUSE "mpdata_plan_diffuse_f32"' in f90 and 'MPDATA_C_DIFFUSE_DEVICE "mpdata_diffuse_f32_device"' in f90


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    ok = [one] * 9
    for fn in (L.mpdata_diffuse_device, L.mpdata_diffuse_f32_device):
        for i, nm in enumerate(("f", "rho", "adz", "tkh", "cx", "cz")):
            args = list(ok)
            args[i] = None
            assert fn(4, 5, 6, 1, 0, 4, *args, None) == mpdata.EINVAL, nm
            assert b"null " + nm.encode() in L.mpdata_last_error()
        assert fn(4, 0, 6, 1, 0, 4, *ok, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, 0, 4, *ok, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(0, 5, 6, 1, 0, 1, *ok, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, 0, 4, *ok, None) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert fn(4, 5, 6, 1, sl0, n, *ok, None) == mpdata.EINVAL, (sl0, n)
            assert b"outside" in L.mpdata_last_error()
    six = [one] * 6
    assert L.mpdata_plan_diffuse_device(None, 0, 1, *six, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_diffuse(None, 0, 1, *six) == mpdata.EINVAL
    assert L.mpdata_plan_diffuse_f32(None, 0, 1, *six) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_diffuse_device(one, sl0, n, *six, 0, 1) == mpdata.EINVAL


def test_new_kernels_do_not_spill():
    """the resource-usage report the build writes next to the object of mpdata_diffuse.hip"""
    rep = os.path.join(ROOT, "codesign-kernels_amd", "csrc", "mpdata_diffuse.usage.txt")
    if not os.path.exists(rep):
        pytest.skip("no resource-usage report (library not built here)")
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_diffuse_kernel", txt)) == 2
    assert len(re.findall(r"Function Name: \S*ref_diffuse_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert scratch and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
