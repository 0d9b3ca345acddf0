"""GPU tests: tall columns (include/mpdata_hip.h section 3e) -- plans, device calls and host calls with nz > 238 as
overlapping level windows of a wave-major plan, every entry point against the CPU oracle on the TALL problem.

Bars:
  * EXACT: f (every element, halo columns included) and flux (all nz levels) equal the oracle bit pattern for bit pattern.
  * FAST: per tracer max|f - f_oracle| <= K * 64 u * max|f_in| and max|flux - flux_oracle| over levels 1..nzm
    <= K * 64 u * max|flux_oracle|, u the unit roundoff of the dtype, K the number of steps taken (the project's
    bound of tests/test_value_regimes.py, whose periodic path scales it by the step count in the same way);
    flux(:, nz) bit for bit.
Several steps feed the oracle its own output (GIVEN plans: the halo columns a run leaves behind are the next step's
inputs); PERIODIC plans are compared with `wrap; advect` per step and a final wrap.  Every test switches the feature
on through the new entry point, so none of them can pass without it.
"""
import numpy as np
import pytest

from plan_harness import upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu

UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
C_FAST = 64.0


def w_of(nz):
    """W by the documented rule, written out again here"""
    return 1 if nz <= 64 else -(-(nz - 1 - 6) // 57)


# nz = 57 j + 7 is the tallest column of j windows: the boundary (that nz, the next) and one more on either side
BOUNDARY_NZ = sorted({57 * j + 7 + d for j in range(5, 18) for d in (-1, 0, 1, 2)})


@pytest.fixture(scope="module")
def M(mpdata):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    return mpdata


@pytest.fixture(autouse=True)
def _tall(mpdata):
    """the switch on for the test; the library's defaults before and after"""
    def reset():
        mpdata.set_tile(-1)
        mpdata.set_wm_flags(0)
        mpdata.set_plan_layout(mpdata.LAYOUT_WAVEMAJOR)
        mpdata.set_variant(mpdata.VARIANT_EXACT)
        mpdata.set_tall_columns(0)
    reset()
    mpdata.set_tall_columns(1)
    yield
    reset()


def make(oracle, shape, T=1, dtype=np.float64, dist=None, seed=100):
    dist = oracle.DIST_CONDITIONED if dist is None else dist
    inp = oracle.make_inputs(*shape, seed=seed, dist=dist, dtype=dtype)
    if T > 1:
        inp["f"] = np.asfortranarray(np.stack(
            [oracle.make_inputs(*shape, seed=seed + 7 * t, dist=dist, dtype=dtype)["f"] for t in range(T)], axis=-1))
        inp["flux"] = np.asfortranarray(np.stack(
            [oracle.make_inputs(*shape, seed=seed + 11 * t, dist=dist, dtype=dtype)["flux"] for t in range(T)], axis=-1))
    return inp


def wrap(f):
    nx = f.shape[1] - 6
    for i in (-2, -1, 0, nx + 1, nx + 2, nx + 3):
        f[:, i + 2] = f[:, 1 + (i - 1) % nx + 2]
    return f


def oracle_steps(oracle, inp, K, periodic=False):
    f, flux = np.array(inp["f"], order="F"), np.array(inp["flux"], order="F")
    for _ in range(K):
        if periodic:
            wrap(f)
        f, flux = oracle.advect(dict(inp, f=f, flux=flux), nthreads=4)
    if periodic:
        wrap(f)
    return f, flux


def _tracers(a, T):
    return [a[..., t] for t in range(T)] if T > 1 else [a]


def check(M, variant, inp, f, flux, f_ref, flux_ref, steps=1, what=""):
    dt = inp["f"].dtype.type
    assert f.dtype == dt and flux.dtype == dt
    if variant == M.VARIANT_EXACT:
        assert_bitwise(f, f_ref, what + " f")
        assert_bitwise(flux, flux_ref, what + " flux")
        return
    T = inp["f"].shape[3] if inp["f"].ndim == 4 else 1
    u = UNIT[dt]
    for t, (fi, ft, flt, fr, flr) in enumerate(zip(_tracers(inp["f"], T), _tracers(f, T), _tracers(flux, T),
                                                   _tracers(f_ref, T), _tracers(flux_ref, T))):
        S = float(np.max(np.abs(fi.astype(np.float64))))
        df = float(np.max(np.abs(ft.astype(np.float64) - fr)))
        nzm = flt.shape[1] - 1
        SF = float(np.max(np.abs(flr[:, :nzm].astype(np.float64))))
        dfl = float(np.max(np.abs(flt[:, :nzm].astype(np.float64) - flr[:, :nzm])))
        print(f"{what} tracer {t}: max|df| = {df / (u * S):.2f} u max|f_in|, max|dflux| = {dfl / (u * SF) if SF else 0:.2f} u max|flux|")
        assert df <= steps * C_FAST * u * S, f"{what} tracer {t}: max|df| = {df:.3e} = {df / (u * S):.1f} u * max|f_in|"
        assert dfl <= steps * C_FAST * u * SF, f"{what} tracer {t}: max|dflux| = {dfl:.3e}, max|flux| = {SF:.3e}"
        assert_bitwise(flt[:, nzm], flr[:, nzm], f"{what} tracer {t} flux(:, nz)")


def dims(inp):
    ncrms, nxp6, nzm = inp["f"].shape[:3]
    return ncrms, nxp6 - 6, nzm + 1, (inp["f"].shape[3] if inp["f"].ndim == 4 else 1)


def new_plan(M, inp, **kw):
    ncrms, nx, nz, T = dims(inp)
    p = M.Plan(ncrms, nx, nz, T, dtype=inp["f"].dtype.type, **kw)
    if not kw:
        assert p.layout == M.LAYOUT_WAVEMAJOR
    assert p.level_windows == w_of(nz) >= 5
    return p


def download(p, inp):
    f, flux = np.empty_like(inp["f"], order="F"), np.empty_like(inp["flux"], order="F")
    p.download(f, flux)
    return f, flux


def plan_steps(M, inp, K, periodic=False):
    p = new_plan(M, inp)
    try:
        upload(p, inp)
        if periodic:
            p.set_boundary(M.BOUNDARY_PERIODIC)
        for _ in range(K):
            p.run()
        p.sync()
        assert p.last_kernel_ms() > 0
        return download(p, inp)
    finally:
        p.close()


VARIANTS = ["exact", "fast"]


def var_of(M, name):
    v = M.VARIANT_EXACT if name == "exact" else M.VARIANT_FAST
    M.set_variant(v)
    return v


# (ncrms, nx, nz): odd and even ncrms, nx 1 / 5 / 37 / 70 (70: the park array of EXACT plans), the first shapes above
# 238 levels, nx = 150 (no kernel of the reference layout covers it above 238 levels)
SHAPES = [(3, 5, 239), (4, 1, 240), (2, 37, 300), (3, 70, 300), (5, 5, 457), (2, 3, 1000), (2, 150, 300), (7, 1, 239)]
SHAPES_F32 = [(4, 5, 300), (2, 37, 300), (2, 5, 239), (4, 3, 240), (6, 1, 457), (2, 70, 300)]   # (239, 240: W = 5, pairs straddle instances)


def _sid(s):
    return "x".join(str(x) for x in s)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_one_run(M, oracle, shape, variant):
    v = var_of(M, variant)
    # the raw law with signed velocities is not a conditioned input: bit equality holds on it, the FAST bound is the
    # library's statement about conditioned inputs (include/mpdata_hip.h, MPDATA_VARIANT_FAST) and is checked on those
    for dist in (oracle.DIST_CONDITIONED, oracle.DIST_RAW_SIGNED)[:2 if v == M.VARIANT_EXACT else 1]:
        inp = make(oracle, shape, dist=dist)
        f, flux = plan_steps(M, inp, 1)
        check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 1), what=f"dist {dist}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nz", BOUNDARY_NZ)
def test_two_runs_at_every_window_count_boundary(M, oracle, nz, variant):
    v = var_of(M, variant)
    inp = make(oracle, (2 + nz % 2, 3, nz))
    f, flux = plan_steps(M, inp, 2)
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 2), steps=2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES_F32, ids=_sid)
def test_fp32_is_the_fp32_oracle(M, oracle, shape, variant):
    """fp32 above 238 levels (an even ncrms): an error without the windows; one run and three"""
    v = var_of(M, variant)
    inp = make(oracle, shape, dtype=np.float32)
    for K in (1, 3):
        f, flux = plan_steps(M, inp, K)
        check(M, v, inp, f, flux, *oracle_steps(oracle, inp, K), steps=K, what=f"{K} runs")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_three_given_runs(M, oracle, shape, variant):
    """the test that sees the seam refresh: the margin levels of every window are wrong after a run"""
    v = var_of(M, variant)
    inp = make(oracle, shape)
    f, flux = plan_steps(M, inp, 3)
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 3), steps=3)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(3, 5, 239), (2, 37, 300), (4, 1, 457), (2, 70, 300)], ids=_sid)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_three_periodic_runs(M, oracle, shape, dtype, variant):
    if dtype == np.float32 and shape[0] % 2:
        shape = (shape[0] + 1,) + shape[1:]
    v = var_of(M, variant)
    inp = make(oracle, shape, dtype=dtype)
    f, flux = plan_steps(M, inp, 3, periodic=True)
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 3, periodic=True), steps=3)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("periodic", [False, True], ids=["given", "periodic"])
def test_tracer_batches_and_sub_ranges(M, oracle, T, periodic, variant):
    """a step of the whole batch, then a step as a sub-range followed by the rest: the seam bytes are per tracer"""
    v = var_of(M, variant)
    inp = make(oracle, (3, 9, 300), T=T)
    p = new_plan(M, inp)
    try:
        upload(p, inp)
        if periodic:
            p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        p.run(1, T - 1)
        p.run(0, 1)
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 2, periodic=periodic), steps=2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_run_uw_then_run_is_a_state_error(M, oracle, dtype, variant):
    v = var_of(M, variant)
    shape = (4, 9, 300)
    inp = make(oracle, shape, T=2, dtype=dtype)
    other = make(oracle, shape, dtype=dtype, seed=977)
    p = new_plan(M, inp)
    try:
        p.upload(inp["f"], other["u"], other["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
        du, dw = to_dev(inp["u"]), to_dev(inp["w"])
        p.run_uw(du, dw)
        p.run_uw(du, dw)
        with pytest.raises(M.MpdataError) as e:
            p.run()
        assert e.value.code == M.ESTATE
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 2), steps=2)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("periodic", [False, True], ids=["given", "periodic"])
def test_instance_blocks_at_unaligned_offsets(M, oracle, dtype, periodic, variant):
    """run; replace a block of f (and of u) that respects nothing; run again (the instances outside the block still
    need their seams refreshed); read back in blocks, on the device and on the host"""
    v = var_of(M, variant)
    n, nx, nz, T = 8, 6, 300, 2
    inp = make(oracle, (n, nx, nz), T=T, dtype=dtype)
    sl0, nb = 1, 5
    blk = make(oracle, (nb, nx, nz), T=T, dtype=dtype, seed=555)
    p = new_plan(M, inp)
    try:
        upload(p, inp)
        if periodic:
            p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        p.import_block(sl0, f=to_dev(blk["f"]), u=to_dev(blk["u"]), flux=to_dev(blk["flux"]))
        p.run()
        p.sync()
        parts = []
        for a, m in ((0, 3), (3, 4), (7, 1)):
            df, dl = to_dev(np.zeros((m, nx + 6, nz - 1, T), dtype, order="F")), to_dev(np.zeros((m, nz, T), dtype, order="F"))
            p.export_block(a, f=df, flux=dl)
            parts.append((to_host(df), to_host(dl)))
        hf, hl = np.empty((4, nx + 6, nz - 1, T), dtype, order="F"), np.empty((4, nz, T), dtype, order="F")
        p.download_block(2, hf, hl)
        f, flux = download(p, inp)
    finally:
        p.close()
    f1, flux1 = oracle_steps(oracle, inp, 1, periodic=periodic)
    mid = dict(inp, f=f1, flux=flux1, u=inp["u"].copy(order="F"))
    mid["f"][sl0:sl0 + nb] = blk["f"]
    mid["flux"][sl0:sl0 + nb] = blk["flux"]
    mid["u"][sl0:sl0 + nb] = blk["u"]
    f_ref, flux_ref = oracle_steps(oracle, mid, 1, periodic=periodic)
    scale = dict(inp, f=np.maximum(np.abs(inp["f"]), np.abs(mid["f"])))   # (FAST: the larger of the two inputs per tracer)
    check(M, v, scale, f, flux, f_ref, flux_ref, steps=2)
    assert_bitwise(np.concatenate([a for a, _ in parts], axis=0), f, "f in blocks")
    assert_bitwise(np.concatenate([b for _, b in parts], axis=0), flux, "flux in blocks")
    assert_bitwise(hf, f[2:6], "download_block f")
    assert_bitwise(hl, flux[2:6], "download_block flux")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype,shape", [(np.float64, (5, 9, 300)), (np.float64, (2, 150, 260)), (np.float32, (4, 9, 300))],
                         ids=["f64", "f64-nx150", "f32"])
def test_device_call(M, oracle, dtype, shape, variant):
    import torch
    v = var_of(M, variant)
    inp = make(oracle, shape, T=2, dtype=dtype)
    d = {k: to_dev(a) for k, a in inp.items()}
    M.advect_scalar2D(d["f"], d["u"], d["w"], d["rho"], d["rhow"], d["flux"], d["adz"])
    torch.cuda.synchronize()
    M.release_host_buffers()
    check(M, v, inp, to_host(d["f"]), to_host(d["flux"]), *oracle_steps(oracle, inp, 1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_call(M, oracle, variant):
    v = var_of(M, variant)
    inp = make(oracle, (6, 150, 260))
    f, flux = inp["f"].copy(order="F"), inp["flux"].copy(order="F")
    M.advect_scalar2D_host(f, inp["u"], inp["w"], inp["rho"], inp["rhow"], flux, inp["adz"])
    M.release_host_buffers()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_create_multi_two_shards_on_one_device(M, oracle, variant):
    v = var_of(M, variant)
    inp = make(oracle, (7, 5, 300), T=2)
    p = new_plan(M, inp, devices=[0, 0])
    try:
        assert p.ngpus == 2 and p.shard_plan(1).level_windows == w_of(300)
        upload(p, inp)
        p.run()
        p.run()
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 2), steps=2)


def test_set_stream_and_timing(M, oracle):
    import torch
    inp = make(oracle, (3, 5, 300))
    p = new_plan(M, inp)
    try:
        upload(p, inp)
        s = torch.cuda.Stream()
        p.set_stream(s)
        p.run()
        p.run()
        p.sync()
        assert p.last_kernel_ms() > 0
        p.set_timing(False)
        p.run()
        with pytest.raises(M.MpdataError) as e:
            p.last_kernel_ms()
        assert e.value.code == M.ESTATE
        s.synchronize()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, M.VARIANT_EXACT, inp, f, flux, *oracle_steps(oracle, inp, 3))


def test_switch_off_and_reference_layout_win(M, oracle):
    assert M.set_tall_columns(0) == 1
    p = M.Plan(3, 5, 239)
    assert p.level_windows == 1 and p.layout == M.LAYOUT_REFERENCE
    p.close()
    with pytest.raises(M.MpdataError) as e:
        M.Plan(4, 5, 300, dtype=np.float32)
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        M.Plan(2, 150, 300)
    assert e.value.code == M.EUNSUPPORTED
    assert M.set_tall_columns(1) == 0
    M.set_plan_layout(M.LAYOUT_REFERENCE)
    p = M.Plan(3, 5, 239)
    assert p.level_windows == 1 and p.layout == M.LAYOUT_REFERENCE
    p.close()
    M.set_plan_layout(M.LAYOUT_WAVEMAJOR)
    for shape in ((3, 5, 238), (3, 5, 64)):   # not affected by the switch
        p = M.Plan(*shape)
        assert p.level_windows == 1 and p.layout == M.LAYOUT_WAVEMAJOR
        p.close()
    with pytest.raises(M.MpdataError) as e:   # fp32 with an odd ncrms stays as it is: no kernel covers it
        M.Plan(3, 5, 300, dtype=np.float32)
    assert e.value.code == M.EUNSUPPORTED


def test_full_size_4096x32x300(M, oracle):
    """the shape a CRM taken from 200 to 300 levels has: blocks of instances against the oracle, the output contract
    (flux(:, nz), f(:, -2), f(:, nx+3) untouched) on the whole arrays"""
    import torch
    n, nx, nz = 4096, 32, 300
    sh = M.shapes(n, nx, nz)
    d = {}
    for k in ("f", "u", "w", "rho", "rhow", "adz", "flux"):
        d[k] = torch.empty(sh[k], dtype=torch.float64, device="cuda:0")
        M.fill_synthetic(d[k], k, 100, oracle.DIST_CONDITIONED)
    torch.cuda.synchronize()
    f_in, flux_in = d["f"].clone(), d["flux"].clone()
    p = M.Plan(n, nx, nz)
    try:
        assert p.level_windows == w_of(nz) and p.layout == M.LAYOUT_WAVEMAJOR
        p.import_device(**d)
        p.run()
        p.run()
        p.export_device(f=d["f"], flux=d["flux"])
        p.sync()
    finally:
        p.close()
    torch.cuda.synchronize()
    # torch axes are reversed: f (nzm, nx+6, ncrms), flux (nz, ncrms)
    assert torch.equal(d["flux"][nz - 1], flux_in[nz - 1]), "flux(:, nz) was written"
    assert torch.equal(d["f"][:, 0], f_in[:, 0]) and torch.equal(d["f"][:, nx + 5], f_in[:, nx + 5]), "f(:, -2) or f(:, nx+3) was written"
    for sl0, m in ((0, 6), (2045, 7), (4090, 6)):
        inp = oracle.make_inputs(m, nx, nz, seed=100, dist=oracle.DIST_CONDITIONED, ncrms_global=n, sl0=sl0)
        f_ref, flux_ref = oracle_steps(oracle, inp, 2)
        assert_bitwise(to_host(d["f"][..., sl0:sl0 + m].contiguous()), f_ref, f"f of instances {sl0}..{sl0 + m - 1}")
        assert_bitwise(to_host(d["flux"][..., sl0:sl0 + m].contiguous()), flux_ref, f"flux of instances {sl0}..{sl0 + m - 1}")
