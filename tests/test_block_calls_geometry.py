"""GPU tests of the six calls on a block of instances (include/mpdata_hip.h 3g .. 3l: level statistics, Courant number,
level increments, velocity scaling, column paths, eddy diffusion) at the sizes the suites of the single calls do not
reach -- those use at most 70 instances, 11 columns, 3 tracers and arrays of a few hundred KB:

  A. the instance axis of the reference-layout kernels beyond one thread block of 256 (array forms, LAYOUT_REFERENCE
     plans, an odd fp32 plan without the switch): ncrms 257, 300, 600 / 601, blocks whose sl0 is no multiple of 256;
  B. the row loop of the same kernels beyond gridDim.y = 65535 (array forms, 3 instances);
  C. the plan-layout kernels at hundreds of tiles and workgroups, with several tracers, blocks that start deep inside
     the plan, and the workload's nx = 32 at nz = 28 (four column batches of the column path);
  D. arrays beyond 2^31 elements and 2^32 bytes: tests/test_block_calls_geometry_big.py.

Every comparison is bit for bit (util.assert_bitwise) against the numpy models of tests/*_model.py applied to the
arrays that were uploaded (block_geometry.Truth); no plan model and no advection run.  A plan's u and w have no export:
velocity scaling is observed through the plan's Courant number of ALL instances after the call.  Outputs lie between
patterned bands of 4 KiB that must come back unchanged, inputs must come back unchanged, and after every in-place call
the plan's WHOLE f (or Courant number) is compared, so everything outside the block and the tracer range keeps its bits.
tests/test_block_calls_geometry_cpu.py asserts, without a GPU, that these inputs are sharp and that each case has the
geometry it is here for."""
import numpy as np
import pytest

import block_geometry as G
import diffuse_model as DM
import level_add_model as AM
import scale_uw_model as SM
from plan_harness import BAND, _defaults, banded, tdt, upload
from test_plan_column_path import paths
from test_plan_courant import cour
from test_plan_level_add import add
from test_plan_level_stats import stats
from test_plan_scale_uw import scale
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
SEED = 700


def same_bits(a, b):
    import torch
    iv = {8: torch.int64, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


def bands_ok(b, what):
    import torch
    raw, pristine, _ = b
    assert torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:]), f"{what}: a band byte changed"


def host_of(view, want):
    """a device output as the Fortran array of the model's shape (same bytes: a dropped or added axis of length 1)"""
    got = to_host(view)
    assert got.size == want.size and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return got.reshape(want.shape, order="F")


def new_plan(M, shape, T, dt, sw):
    M.set_plan_layout(M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    return M.Plan(*shape, T, dtype=dt)


def export_f(M, p, shape, T, dt):
    """the plan's whole f, with the tracer axis"""
    import torch
    f = torch.empty(M.shapes(*shape, T)["f"], dtype=tdt(dt), device="cuda:0")
    p.export_device(f=f)
    p.sync()
    h = to_host(f)
    return h.reshape(h.shape + (() if T > 1 else (1,)), order="F")


def plan_diffuse(p, shape, dt, c, sl0, n, first, ntr):
    """Plan.diffuse of host coefficients c -> zflux (n, nz, ntr); the inputs and the bands of zflux are checked"""
    import torch
    dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
    orig = {k: None if v is None else v.clone() for k, v in dev.items()}
    zb = banded((ntr, shape[2], n), dt)
    torch.cuda.synchronize()
    p.diffuse(dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2], sl0, n, first, ntr)
    p.sync()
    for k, v in dev.items():
        assert v is None or same_bits(v, orig[k]), f"{k} changed"
    bands_ok(zb, "zflux")
    return to_host(zb[2])


def check_six(M, p, tr, what, sl0, n, first, ntr, k, windowed=False):
    """the six calls on block [sl0, sl0 + n), tracers [first, first + ntr) of plan p, which holds what tr holds"""
    shape, T, dt = tr.shape, tr.T, tr.dt
    ncrms, nx, nz = shape
    what = f"{what} block {sl0, n} tracers {first, ntr}"
    # 3g, 3h, 3k: read-only
    got, want = stats(p, dt, nz - 1, sl0, n, first, ntr), tr.stats(sl0, n, first, ntr)
    for key in want:
        assert_bitwise(got[key], want[key], f"{what}: {key}")
    got, want = cour(p, dt, nz - 1, sl0, n), tr.courant(sl0, n)
    for key in want:
        assert_bitwise(got[key], want[key], f"{what}: {key}")
    got, want = paths(M, p, dt, nx, sl0, n, first, ntr), tr.paths(sl0, n, first, ntr)
    assert_bitwise(got[0], want[0], f"{what}: path")
    assert_bitwise(got[1], want[1], f"{what}: mass")
    # 3i: the whole f afterwards (the read-only calls before it changed nothing either)
    d = G.make_d(shape, ntr, dt, 300 + k, n)
    add(p, d, sl0, n, AM.ADD, first)
    tr.add(d, sl0, n, first, ntr)
    assert_bitwise(export_f(M, p, shape, T, dt), tr.f, f"{what}: f after level_add")
    # 3j: through the Courant number of every instance
    su = None if k % 3 == 2 else SM.make_s(shape, dt, 400 + k, n)
    sw = None if k % 3 == 1 else SM.make_s(shape, dt, 1400 + k, n)
    scale(p, su, sw, sl0, n)
    tr.scale(su, sw, sl0, n)
    got, want = cour(p, dt, nz - 1, 0, ncrms), tr.courant()
    for key in want:
        assert_bitwise(got[key], want[key], f"{what}: {key} of the whole plan after scale_uw")
    # 3l: both surface fluxes in the even calls, neither in the odd ones
    c = DM.make_coeffs(n, nx, nz, dt, 500 + k, fluxes=k % 2 == 0)
    if windowed:
        with pytest.raises(M.MpdataError) as e:
            plan_diffuse(p, shape, dt, c, sl0, n, first, ntr)
        assert e.value.code == M.EUNSUPPORTED
    else:
        z = plan_diffuse(p, shape, dt, c, sl0, n, first, ntr)
        assert_bitwise(z, tr.diffuse(c, sl0, n, first, ntr), f"{what}: zflux")
    assert_bitwise(export_f(M, p, shape, T, dt), tr.f, f"{what}: f after diffuse")


def clip_whole(M, p, tr, what):
    """MPDATA_LEVEL_ADD_CLIP on the whole plan, last: the sign of its zeros is unspecified, so nothing is computed from them"""
    d = G.make_d(tr.shape, tr.T, tr.dt, 399, tr.shape[0])
    add(p, d, 0, tr.shape[0], AM.CLIP, 0)
    tr.add(d, clip=True)
    assert np.any(tr.f == 0) and np.any(tr.f > 0)
    assert_bitwise(AM.canon(export_f(M, p, tr.shape, tr.T, tr.dt)), AM.canon(tr.f), f"{what}: f after level_add CLIP")


def resolve(block, ncrms):
    sl0, n = block
    sl0 = ncrms + sl0 if sl0 < 0 else sl0
    return sl0, (ncrms - sl0 if n is None else n)


# ---- A. the instance axis of the reference-layout kernels
@pytest.mark.parametrize("name", list(G.REF_KINDS))
def test_a_reference_layout_plans(mpdata, name):
    M = mpdata
    shape, T, dt, sw, blocks = G.REF_KINDS[name]
    inp = G.make_inputs(shape, T, dt, SEED)
    p = new_plan(M, shape, T, dt, sw)
    assert p.layout == M.LAYOUT_REFERENCE, name
    upload(p, G.plan_arrays(inp))
    tr = G.Truth(inp)
    for k, blk in enumerate(blocks):
        sl0, n = resolve(blk, shape[0])
        if k == 0 or blk in ((200, 300), (30, 270)):         # more than one thread block
            assert n > G.TB and (k or n == shape[0]), (name, blk)
        first, ntr = ((0, T), (1, 1), (0, 1))[k % 3]
        check_six(M, p, tr, name, sl0, n, first, ntr, k)
    clip_whole(M, p, tr, name)
    p.close()


def array_forms(M, inp, which, blocks=((0, None),), squeeze=False):
    """the array forms named in `which` on the device copies of inp (squeeze: one tracer without the tracer axis); the
    diffusion on every block of `blocks`"""
    import torch
    tr = G.Truth(inp)
    (ncrms, nx, nz), T, dt = tr.shape, tr.T, tr.dt
    nzm = nz - 1
    assert not squeeze or T == 1
    lead = () if squeeze else (T,)
    dev_f = lambda: to_dev(np.asfortranarray(tr.f[..., 0]) if squeeze else tr.f)
    rho, adz = to_dev(tr.rho), to_dev(tr.adz)
    rho0, adz0 = rho.clone(), adz.clone()
    if "stats" in which:
        f = dev_f()
        keep = f.clone()
        bufs = {k: banded(lead + (nzm, ncrms), dt) for k in ("sum", "min", "max")}
        torch.cuda.synchronize()
        M.level_stats(f, **{k: b[2] for k, b in bufs.items()})
        torch.cuda.synchronize()
        assert same_bits(f, keep), "level_stats changed f"
        for k, want in tr.stats().items():
            bands_ok(bufs[k], k)
            assert_bitwise(host_of(bufs[k][2], want), want, f"array form level_stats: {k}")
    if "courant" in which:
        u, w = to_dev(tr.u), to_dev(tr.w)
        u0, w0 = u.clone(), w.clone()
        bufs = {"clev": banded((nzm, ncrms), dt), "cinst": banded((ncrms,), dt)}
        torch.cuda.synchronize()
        M.courant(u, w, rho, adz, bufs["clev"][2], bufs["cinst"][2])
        torch.cuda.synchronize()
        assert same_bits(u, u0) and same_bits(w, w0), "courant changed u or w"
        for k, want in tr.courant().items():
            bands_ok(bufs[k], k)
            assert_bitwise(host_of(bufs[k][2], want), want, f"array form courant: {k}")
    if "path" in which:
        f = dev_f()
        keep = f.clone()
        sh = M.column_path_shapes(ncrms, nx, None if squeeze else T)
        bufs = {k: banded(sh[k], dt) for k in ("path", "mass")}
        torch.cuda.synchronize()
        M.column_path(f, rho, adz, bufs["path"][2], bufs["mass"][2])
        torch.cuda.synchronize()
        assert same_bits(f, keep), "column_path changed f"
        for k, want in zip(("path", "mass"), tr.paths()):
            bands_ok(bufs[k], k)
            assert_bitwise(host_of(bufs[k][2], want), want, f"array form column_path: {k}")
    if "level_add" in which:
        f = dev_f()
        d = G.make_d(tr.shape, T, dt, 300, ncrms)
        db = banded(lead + (nzm, ncrms), dt)
        db[2].copy_(to_dev(d).view(db[2].shape))
        torch.cuda.synchronize()
        pristine = db[0].clone()
        M.level_add(f, db[2], AM.ADD)
        torch.cuda.synchronize()
        assert torch.equal(db[0], pristine), "a byte of d or of its bands changed"
        tr.add(d)
        assert_bitwise(host_of(f, tr.f), tr.f, "array form level_add: f")
    if "scale" in which:
        u, w = to_dev(tr.u), to_dev(tr.w)
        su, sw = SM.make_s(tr.shape, dt, 400), SM.make_s(tr.shape, dt, 1400)
        dsu, dsw = torch.from_numpy(su).to("cuda:0"), torch.from_numpy(sw).to("cuda:0")
        M.scale_uw(u, w, dsu, dsw)
        torch.cuda.synchronize()
        assert same_bits(dsu, torch.from_numpy(su).to("cuda:0")) and same_bits(dsw, torch.from_numpy(sw).to("cuda:0"))
        tr.scale(su, sw)
        assert_bitwise(to_host(u), tr.u, "array form scale_uw: u")
        assert_bitwise(to_host(w), tr.w, "array form scale_uw: w")
    if "diffuse" in which:
        for k, blk in enumerate(blocks):
            sl0, n = resolve(blk, ncrms)
            f = dev_f()
            c = DM.make_coeffs(n, nx, nz, dt, 500 + k, fluxes=k % 2 == 0)
            dev = {key: None if v is None else to_dev(v) for key, v in c.items()}
            orig = {key: None if v is None else v.clone() for key, v in dev.items()}
            zb = banded(lead + (nz, n), dt)
            torch.cuda.synchronize()
            M.diffuse(f, rho, adz, dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2], sl0, n)
            torch.cuda.synchronize()
            for key, v in dev.items():
                assert v is None or same_bits(v, orig[key]), f"{key} changed"
            bands_ok(zb, "zflux")
            want = tr.diffuse(c, sl0, n)
            assert_bitwise(host_of(zb[2], want), want, f"array form diffuse {sl0, n}: zflux")
            assert_bitwise(host_of(f, tr.f), tr.f, f"array form diffuse {sl0, n}: f")
    assert same_bits(rho, rho0) and same_bits(adz, adz0), "rho or adz changed"


ALL_SIX = ("stats", "courant", "path", "level_add", "scale", "diffuse")


@pytest.mark.parametrize("ncrms,dt", G.ARRAY_A, ids=[f"{'f64' if dt == G.F64 else 'f32'}-n{n}" for n, dt in G.ARRAY_A])
def test_a_array_forms(mpdata, ncrms, dt):
    nx, nz = G.ARRAY_A_SHAPE[ncrms]
    assert ncrms > G.TB
    inp = G.make_inputs((ncrms, nx, nz), 2, dt, SEED + 1)
    array_forms(mpdata, inp, ALL_SIX, G.BLOCKS_600 if ncrms == 600 else [(0, None), (1, 256)])


# ---- B. the row loop of the reference-layout kernels
@pytest.mark.parametrize("dt", [G.F64, G.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(G.ROW_CASES))
def test_b_row_loop(mpdata, case, dt):
    """rows in (65535, 66000]: the second trip of `for (r = blockIdx.y; r < rows; r += gridDim.y)`.  No array form's
    validation refuses such a shape: the second trip is reachable for every kernel (the mass pass at 65537 tracers)."""
    shape, T = G.ROW_CASES[case]
    rows = G.rows_of(case)
    assert rows and all(G.YMAX < r <= 66000 for r in rows.values()), rows
    which = {"f-rows": ("stats", "level_add", "diffuse"), "uw-rows": ("courant", "scale"), "path-": ("path",)}
    which = [v for k, v in which.items() if case.startswith(k)][0]
    inp = G.make_inputs(shape, T, dt, SEED + 2)
    array_forms(mpdata, inp, which, squeeze=case == "f-rows-one-tracer")


# ---- C. the plan-layout kernels at hundreds of workgroups
@pytest.mark.parametrize("name", list(G.WM_KINDS))
def test_c_wave_major_plans(mpdata, name):
    M = mpdata
    shape, T, dt, sw, blocks = G.WM_KINDS[name]
    inp = G.make_inputs(shape, T, dt, SEED + 3)
    p = new_plan(M, shape, T, dt, sw)
    assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == bool(sw.get("tall")), name
    upload(p, G.plan_arrays(inp))
    tr = G.Truth(inp)
    for k, (sl0, n, first, ntr) in enumerate(blocks):
        check_six(M, p, tr, name, sl0, n, first, ntr, k, windowed=bool(sw.get("tall")))
    clip_whole(M, p, tr, name)
    p.close()


def test_c_host_forms_grow_the_staging_buffer(mpdata):
    """the six host forms on the 601-instance fp64 plan: a block of 5 instances, then one of 400 (> 256), so the plan's
    block staging buffer is freed and allocated anew between two calls"""
    M = mpdata
    name = "f64-n601-nx32-nz28"
    shape, T, dt, sw, _ = G.WM_KINDS[name]
    ncrms, nx, nz = shape
    inp = G.make_inputs(shape, T, dt, SEED + 3)
    p = new_plan(M, shape, T, dt, sw)
    upload(p, G.plan_arrays(inp))
    tr = G.Truth(inp)
    for k, (sl0, n) in enumerate(((3, 5), (100, 400))):
        what = f"{name} host forms {sl0, n}"
        assert k == 0 or n > G.TB
        out = {key: np.full((n, nz - 1, T), -7, dt, order="F") for key in ("sum", "min", "max")}
        p.level_stats_host(sl0, n, **out)
        for key, want in tr.stats(sl0, n).items():
            assert_bitwise(out[key], want, f"{what}: {key}")
        clev, cinst = p.courant_host(sl0, n)
        want = tr.courant(sl0, n)
        assert_bitwise(clev, want["clev"], f"{what}: clev")
        assert_bitwise(cinst, want["cinst"], f"{what}: cinst")
        path, mass = np.full((n, nx, T), -7, dt, order="F"), np.full((n, T), -7, dt, order="F")
        p.column_path_host(path, mass, sl0, n)
        want = tr.paths(sl0, n)
        assert_bitwise(path, want[0], f"{what}: path")
        assert_bitwise(mass, want[1], f"{what}: mass")
        d = G.make_d(shape, T, dt, 310 + k, n)
        d0 = d.copy(order="F")
        p.level_add_host(d, sl0, n)
        assert_bitwise(d, d0, f"{what}: d")
        tr.add(d, sl0, n)
        assert_bitwise(export_f(M, p, shape, T, dt), tr.f, f"{what}: f after level_add")
        su, sw_ = SM.make_s(shape, dt, 410 + k, n), SM.make_s(shape, dt, 1410 + k, n)
        p.scale_uw_host(su, sw_, sl0, n)
        tr.scale(su, sw_, sl0, n)
        got, want = cour(p, dt, nz - 1, 0, ncrms), tr.courant()
        for key in want:
            assert_bitwise(got[key], want[key], f"{what}: {key} of the whole plan after scale_uw")
        c = DM.make_coeffs(n, nx, nz, dt, 510 + k)
        c0 = {key: v.copy(order="F") for key, v in c.items()}
        z = np.full((n, nz, T), -7, dt, order="F")
        p.diffuse_host(c["tkh"], c["cx"], c["cz"], c["sb"], c["st"], z, sl0, n)
        for key in c:
            assert_bitwise(c[key], c0[key], f"{what}: {key}")
        assert_bitwise(z, tr.diffuse(c, sl0, n), f"{what}: zflux")
        assert_bitwise(export_f(M, p, shape, T, dt), tr.f, f"{what}: f after diffuse")
    p.close()
