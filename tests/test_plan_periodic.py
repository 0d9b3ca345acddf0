"""Periodic lateral boundaries of plans (include/mpdata_hip.h 3a) and the device halo helper (3c) on the
GPU.  The yardstick is the oracle loop the boundary mode promises:

    for each run: wrap(f); f, flux = oracle.advect(...)
    wrap(f)

EXACT plans must equal it bit for bit (f with every halo column, flux), FAST plans within K * 1e-12,
on every path a plan can take: the one-tracer kernel, tracer batches and the odd-tracer fold, nx
without the register park, the 65..238-level windows, reference-layout plans, fp32 (wave-major with
an even ncrms, reference layout with an odd one), run_uw, run_tracers, multi-GPU plans."""
import numpy as np
import pytest

from test_periodic_api import MASS_DRIFT_PER_STEP, conserving_inputs, mass, wrap

pytestmark = pytest.mark.gpu


def _inputs(oracle, ncrms, nx, nz, T=1, seed=100, dtype=np.float64):
    inp = oracle.make_inputs(ncrms, nx, nz, seed=seed, dist=oracle.DIST_CONDITIONED, dtype=dtype)
    if T > 1:
        inp["f"] = np.asfortranarray(np.stack(
            [oracle.make_inputs(ncrms, nx, nz, seed=seed + t, dist=oracle.DIST_CONDITIONED, dtype=dtype)["f"]
             for t in range(T)], axis=-1))
        inp["flux"] = np.asfortranarray(np.stack([inp["flux"]] * T, axis=-1))
    return inp


def oracle_loop(oracle, inp, K, nthreads=1):
    f, flux = np.array(inp["f"], order="F"), np.array(inp["flux"], order="F")
    for _ in range(K):
        wrap(f=f)
        f, flux = oracle.advect(dict(inp, f=f, flux=flux), nthreads=nthreads)
    wrap(f=f)
    return f, flux


class _Settings:
    """variant / default layout for the plans created inside the block; restored afterwards"""

    def __init__(self, M, variant, layout=None):
        self.M, self.variant, self.layout = M, variant, layout

    def __enter__(self):
        self.pv = self.M.set_variant(self.variant)
        self.pl = self.M.set_plan_layout(self.layout) if self.layout is not None else None
        return self

    def __exit__(self, *a):
        self.M.set_variant(self.pv)
        if self.pl is not None:
            self.M.set_plan_layout(self.pl)


def plan_loop(M, inp, K, T=1, **kw):
    ncrms, nxp6, nzm = inp["f"].shape[:3]
    p = M.Plan(ncrms, nxp6 - 6, nzm + 1, T, dtype=inp["f"].dtype, **kw)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert p.boundary == M.BOUNDARY_PERIODIC
    for _ in range(K):
        p.run()
    p.sync()
    f, flux = np.empty_like(inp["f"], order="F"), np.empty_like(inp["flux"], order="F")
    p.download(f, flux)
    layout = p.layout
    p.close()
    return f, flux, layout


# (ncrms, nx, nz, T, dtype, layout forced, layout expected)
CASES = [
    ((64, 32, 28), 1, np.float64, None, 1),     # the headline one-tracer kernel (register park)
    ((64, 32, 28), 3, np.float64, None, 1),     # tracer batch + odd-tracer fold
    ((40, 1, 12), 1, np.float64, None, 1),
    ((40, 2, 12), 3, np.float64, None, 1),
    ((40, 3, 12), 1, np.float64, None, 1),
    ((24, 67, 20), 1, np.float64, None, 1),     # nx 67: no register park
    ((48, 9, 8), 1, np.float64, None, 1),
    ((24, 9, 64), 2, np.float64, None, 1),
    ((8, 7, 72), 1, np.float64, None, 1),       # 65..238 levels: windows, tail
    ((6, 5, 130), 3, np.float64, None, 1),
    ((30, 11, 28), 2, np.float64, 0, 0),        # reference-layout plan
    ((8, 5, 240), 1, np.float64, None, 0),      # nz > 238: reference layout
    ((64, 32, 28), 1, np.float32, None, 1),     # fp32, even ncrms: wave-major
    ((33, 10, 20), 3, np.float32, None, 0),     # fp32, odd ncrms: reference layout
]
K = 6


def _id(c):
    (n, nx, nz), T, dt, lay, _ = c
    return f"{n}x{nx}x{nz}-T{T}-{np.dtype(dt).name}" + ("-ref" if lay == 0 else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_periodic_bitwise(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, lay, want_layout = case
    inp = _inputs(oracle, *shape, T=T, dtype=dt)
    with _Settings(M, M.VARIANT_EXACT, lay):
        f, flux, layout = plan_loop(M, inp, K, T)
    assert layout == want_layout
    f_ref, flux_ref = oracle_loop(oracle, inp, K)
    assert np.array_equal(f, f_ref), f"f: max|d|={np.abs(f - f_ref).max():.3e}"
    assert np.array_equal(flux, flux_ref), f"flux: max|d|={np.abs(flux - flux_ref).max():.3e}"


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == np.float64], ids=_id)
def test_fast_periodic_close(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, lay, _ = case
    inp = _inputs(oracle, *shape, T=T, dtype=dt)
    with _Settings(M, M.VARIANT_FAST, lay):
        f, _, _ = plan_loop(M, inp, K, T)
    f_ref, _ = oracle_loop(oracle, inp, K)
    d = float(np.abs(f - f_ref).max())
    assert d <= K * 1e-12, d
    nx = shape[1]
    halo = [0, 1, 2, nx + 3, nx + 4, nx + 5]
    f2 = np.array(f, order="F")
    wrap(f=f2)
    assert np.array_equal(f2[:, halo], f[:, halo])   # read back wrapped, exactly


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda:0")


@pytest.mark.parametrize("shape,T", [((64, 32, 28), 1), ((64, 9, 20), 3), ((33, 8, 28), 1)],
                         ids=["ring", "batch", "convert-odd-ncrms"])
def test_run_uw_periodic_bitwise(mpdata, oracle, shape, T):
    M = mpdata
    inp = _inputs(oracle, *shape, T=T)
    steps = 4
    with _Settings(M, M.VARIANT_EXACT):
        p = M.Plan(*shape, T)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    p.set_boundary(M.BOUNDARY_PERIODIC)
    f, flux = np.array(inp["f"], order="F"), np.array(inp["flux"], order="F")
    for s in range(steps):
        fresh = oracle.make_inputs(*shape, seed=500 + s, dist=oracle.DIST_CONDITIONED)
        wrap(u=fresh["u"], w=fresh["w"])
        du, dw = _dev(fresh["u"]), _dev(fresh["w"])
        p.run_uw(du, dw)
        p.sync()
        wrap(f=f)
        f, flux = oracle.advect(dict(inp, f=f, flux=flux, u=fresh["u"], w=fresh["w"]))
    wrap(f=f)
    g, gl = np.empty_like(f, order="F"), np.empty_like(flux, order="F")
    p.download(g, gl)
    p.close()
    assert np.array_equal(g, f), f"f: max|d|={np.abs(g - f).max():.3e}"
    assert np.array_equal(gl, flux)


def test_run_tracers_subrange(mpdata, oracle):
    M = mpdata
    shape, T = (64, 12, 20), 3
    inp = _inputs(oracle, *shape, T=T)
    with _Settings(M, M.VARIANT_EXACT):
        p = M.Plan(*shape, T)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run(1, 1)
    p.run(1, 1)
    p.sync()
    f, flux = np.empty_like(inp["f"], order="F"), np.empty_like(inp["flux"], order="F")
    p.download(f, flux)
    p.close()
    nx = shape[1]
    for t in (0, 2):   # never run: interior untouched, halos read back wrapped
        assert np.array_equal(f[:, 3:nx + 3, :, t], inp["f"][:, 3:nx + 3, :, t])
        g = np.array(inp["f"][..., t], order="F")
        wrap(f=g)
        assert np.array_equal(f[..., t], g)
    one = dict(inp, f=np.asfortranarray(inp["f"][..., 1]), flux=np.asfortranarray(inp["flux"][..., 1]))
    f_ref, flux_ref = oracle_loop(oracle, one, 2)
    assert np.array_equal(f[..., 1], f_ref)
    assert np.array_equal(flux[..., 1], flux_ref)


def test_mode_switching(mpdata, oracle):
    M = mpdata
    shape = (64, 32, 28)
    inp = _inputs(oracle, *shape)
    with _Settings(M, M.VARIANT_EXACT):
        p = M.Plan(*shape)
        q = M.Plan(*shape)
    for x in (p, q):
        x.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    assert q.boundary == M.BOUNDARY_GIVEN
    # never switched: today's behaviour, two plain oracle calls in a row
    q.run(); q.run(); q.sync()
    f, flux = np.empty_like(inp["f"], order="F"), np.empty_like(inp["flux"], order="F")
    q.download(f, flux)
    q.close()
    a, _ = oracle.advect(inp)
    b, bl = oracle.advect(dict(inp, f=a))
    assert np.array_equal(f, b) and np.array_equal(flux, bl)
    # GIVEN -> PERIODIC (2 runs) -> GIVEN (1 run): the switch back wraps, then a plain step
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run(); p.run()
    p.set_boundary(M.BOUNDARY_GIVEN)
    assert p.boundary == M.BOUNDARY_GIVEN
    p.run(); p.sync()
    p.download(f, flux)
    p.close()
    g, gl = oracle_loop(oracle, inp, 2)
    g, gl = oracle.advect(dict(inp, f=g, flux=gl))
    assert np.array_equal(f, g) and np.array_equal(flux, gl)
    with pytest.raises(M.MpdataError):
        M.Plan(*shape).set_boundary(2)


def test_import_between_runs_rearms_the_refresh(mpdata, oracle):
    import torch
    M = mpdata
    shape = (64, 16, 28)
    inp = _inputs(oracle, *shape)
    other = _inputs(oracle, *shape, seed=321)
    with _Settings(M, M.VARIANT_EXACT):
        p = M.Plan(*shape)
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run()
    fo = np.array(other["f"], order="F")
    nx = shape[1]
    fo[:, [0, 1, 2, nx + 3, nx + 4, nx + 5]] = 1e6   # imported halos are ignored
    p.import_device(f=_dev(fo))
    p.run(); p.run()
    d = torch.empty_like(_dev(fo))
    p.export_device(f=d)
    p.sync()
    g = np.asfortranarray(d.cpu().numpy().T)
    p.close()
    ref, _ = oracle_loop(oracle, dict(inp, f=fo), 2)
    assert np.array_equal(g, ref)


@pytest.mark.parametrize("xfer", ["p2p", "direct"])
def test_multi_gpu_periodic_equals_single(mpdata, oracle, monkeypatch, xfer):
    M = mpdata
    monkeypatch.setenv("MPDATA_MULTI_XFER", xfer)
    shape, T = (131, 32, 28), 2
    inp = _inputs(oracle, *shape, T=T)
    with _Settings(M, M.VARIANT_EXACT):
        f1, fl1, _ = plan_loop(M, inp, 3, T)
        f2, fl2, _ = plan_loop(M, inp, 3, T, devices=[0, 0])
    assert np.array_equal(f2, f1) and np.array_equal(fl2, fl1)
    f_ref, _ = oracle_loop(oracle, inp, 3)
    assert np.array_equal(f1, f_ref)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_helper_equals_numpy_wrap(mpdata, oracle, dt):
    import torch
    M = mpdata
    for shape, T in (((37, 5, 12), 3), ((64, 1, 8), 1), ((20, 32, 28), 1)):
        inp = _inputs(oracle, *shape, T=T, dtype=dt, seed=7)
        dev = {k: _dev(inp[k]) for k in ("f", "u", "w")}
        M.periodic_halo(f=dev["f"], u=dev["u"], w=dev["w"])
        torch.cuda.synchronize()
        want = {k: np.array(inp[k], order="F") for k in ("f", "u", "w")}
        wrap(**want)
        for k in ("f", "u", "w"):
            assert np.array_equal(np.asfortranarray(dev[k].cpu().numpy().T), want[k]), (shape, k)
        # one array alone; the others are left as they are
        du = _dev(inp["u"])
        M.periodic_halo(u=du)
        torch.cuda.synchronize()
        assert np.array_equal(np.asfortranarray(du.cpu().numpy().T), want["u"])


def test_full_size_exact(mpdata, oracle):
    M = mpdata
    shape, steps = (65536, 32, 28), 3
    inp = _inputs(oracle, *shape)
    with _Settings(M, M.VARIANT_EXACT):
        f, flux, _ = plan_loop(M, inp, steps)
    f_ref, flux_ref = oracle_loop(oracle, inp, steps, nthreads=max(1, min(16, oracle.max_threads())))
    nx = shape[1]
    halo = [0, 1, 2, nx + 3, nx + 4, nx + 5]
    assert np.array_equal(f[:, halo], f_ref[:, halo])
    for s0 in (0, 4096, 30000, 65536 - 512):
        assert np.array_equal(f[s0:s0 + 512], f_ref[s0:s0 + 512]), s0
        assert np.array_equal(flux[s0:s0 + 512], flux_ref[s0:s0 + 512]), s0


@pytest.mark.parametrize("variant", ["EXACT", "FAST"])
def test_conservation_and_positivity(mpdata, oracle, variant):
    M = mpdata
    steps = 200
    inp = conserving_inputs(oracle, 4096, 32, 28)
    with _Settings(M, getattr(M, "VARIANT_" + variant)):
        f, _, _ = plan_loop(M, inp, steps)
    m0 = mass(inp["f"], inp)
    drift = float(np.max(np.abs(mass(f, inp) - m0) / np.abs(m0)))
    assert drift <= MASS_DRIFT_PER_STEP * steps, drift
    assert f.min() >= 0
