"""GPU tests: every kernel path on the value regimes of oracle/regimes.py (tiny and large magnitudes, sparse and
front-like fields, zero and signed-zero velocities, mixed scales across tracers and across the instances of an fp32
pair, subnormal fp32).  The parity tests elsewhere feed unit-scale dense fields only, where the limiter's eps cannot be
seen in fp32 and an absolute error bound hides a relative error of 1e-3 at a scale of 1e-12.

Bars, per path and regime:
  * EXACT: f and flux equal the oracle (itself pinned to the reference on these regimes by test_oracle_regimes.py)
    bit pattern for bit pattern, whole arrays: +0.0 and -0.0 differ.  One named exception: on the signed_zero regime
    f may hold zeros of the other sign (every mismatch a (+0, -0) pair; see assert_bitwise_but_zero_sign), on every
    path; flux stays bit-identical there too.
  * FAST, scale-relative, per tracer: max|f - f_oracle| <= C * u * max|f_in| with u the unit roundoff of the dtype;
    flux(:, 1:nzm) likewise against max|flux_oracle(:, 1:nzm)|; flux(:, nz) bit for bit (it is never written).
    C = 64, fixed from the first run on an MI355X, which measured worst ratios (per step) of 32 u for f in fp64 (fronts,
    periodic plan; 8 on the scaled regimes), 16 u in fp32 (fronts, tile 32; 6 elsewhere), 5.4 u for flux(:, 1:nzm).
  * FAST fp32 against the fp64 oracle on the same inputs (it computes the same function: (double)1.e-10f is the fp32
    eps): max|f - hi| <= 2 * max|f_oracle32 - hi| + 4 * u32 * max|f_in|, i.e. FAST fp32 is as accurate as the
    reference's own fp32 build at every scale.
The periodic path runs 4 steps: its FAST bounds are 4 times the one-step ones.
"""
import numpy as np
import pytest

from util import assert_bitwise, bit_mismatches, to_dev

pytestmark = pytest.mark.gpu

C_FAST = 64.0
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
PERIODIC_STEPS = 4

# (id, dtype, (ncrms, nx, nz), ntracers, kind, options)
PATHS = (
    [(f"device-f64-tile{t}", np.float64, (9, 16, 28), 1, "device", {"tile": t}) for t in (0, 1, 2, 3, 4, 22, 23, 24)]
    + [(f"device-f32-tile{t}", np.float32, (9, 16, nz), 1, "device", {"tile": t}) for t, nz in ((30, 8), (31, 16), (32, 28))]
    + [(f"device-f32-tile{t}", np.float32, (10, 16, nz), 1, "device", {"tile": t})
       for t, nz in ((40, 8), (41, 16), (42, 28), (43, 58))]
    + [("device-f64-nz72", np.float64, (5, 9, 72), 1, "device", {}),
       ("plan-wm-stream", np.float64, (10, 16, 28), 1, "plan", {"layout": 1}),
       ("plan-wm-nostream", np.float64, (10, 16, 28), 1, "plan", {"layout": 1, "flags": "WMF_NOSTREAM"}),
       ("plan-wm-batch-T3", np.float64, (10, 16, 28), 3, "plan", {"layout": 1}),
       ("plan-wm-tpw1-T2", np.float64, (10, 16, 28), 2, "plan", {"layout": 1, "flags": "WMF_TPW1"}),
       ("plan-wm-nx67", np.float64, (6, 67, 20), 1, "plan", {"layout": 1}),
       ("plan-wm-nz72", np.float64, (7, 9, 72), 1, "plan", {"layout": 1}),
       ("plan-wm-nz130", np.float64, (4, 7, 130), 1, "plan", {"layout": 1}),
       ("plan-wm-f32", np.float32, (10, 16, 28), 1, "plan", {"layout": 1}),
       ("plan-ref", np.float64, (9, 16, 28), 1, "plan", {"layout": 0, "force_layout": True}),
       ("plan-ref-nz240", np.float64, (3, 5, 240), 1, "plan", {"layout": 0}),
       ("plan-ref-f32-odd", np.float32, (9, 16, 20), 1, "plan", {"layout": 0}),
       ("run_uw-aligned", np.float64, (10, 16, 28), 1, "run_uw", {"misalign": False}),
       ("run_uw-unaligned", np.float64, (10, 16, 28), 1, "run_uw", {"misalign": True}),
       ("plan-periodic", np.float64, (8, 12, 20), 1, "periodic", {}),
       ("host", np.float64, (9, 16, 28), 1, "host", {})])


@pytest.fixture(scope="module")
def R(oracle):
    from oracle import regimes
    return regimes


@pytest.fixture(scope="module")
def M(mpdata):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    yield mpdata


@pytest.fixture(autouse=True)
def _defaults(mpdata):
    """every test starts from, and leaves behind, the library's default launch settings"""
    def reset():
        mpdata.set_tile(-1)
        mpdata.set_wm_flags(0)
        mpdata.set_plan_layout(mpdata.LAYOUT_WAVEMAJOR)
        mpdata.set_variant(mpdata.VARIANT_EXACT)
    reset()
    yield
    reset()


_inputs, _refs = {}, {}
FAST_WORST = {}   # (dtype name, regime) -> worst FAST ratio for f, flux, and against the fp64 oracle


def inputs(R, regime, dtype, shape, ntr):
    key = (regime, np.dtype(dtype).name, shape, ntr)
    if key not in _inputs:
        _inputs[key] = R.make(regime, *shape, seed=100, dtype=dtype, ntracers=ntr)
    return _inputs[key]


def reference(oracle, key, inp, periodic):
    """oracle result on inp (periodic: the wrap + step loop of test_plan_periodic.py), cached per module"""
    if key not in _refs:
        if periodic:
            from test_plan_periodic import oracle_loop
            _refs[key] = oracle_loop(oracle, inp, PERIODIC_STEPS, nthreads=4)
        else:
            _refs[key] = oracle.advect(inp, nthreads=4)
    return _refs[key]


def _host_out(inp):
    return np.empty_like(inp["f"], order="F"), np.empty_like(inp["flux"], order="F")


def run_path(M, oracle, kind, opts, inp, ntr):
    import torch
    ncrms, nxp6, nzm = inp["f"].shape[:3]
    nx, nz = nxp6 - 6, nzm + 1
    dt = inp["f"].dtype.type
    if kind == "device":
        if "tile" in opts:
            M.set_tile(opts["tile"])
        d = {k: to_dev(v) for k, v in inp.items()}
        M.advect_scalar2D(d["f"], d["u"], d["w"], d["rho"], d["rhow"], d["flux"], d["adz"])
        torch.cuda.synchronize()
        return np.asfortranarray(d["f"].cpu().numpy().T), np.asfortranarray(d["flux"].cpu().numpy().T)
    if kind == "host":
        f, flux = inp["f"].copy(order="F"), inp["flux"].copy(order="F")
        M.advect_scalar2D_host(f, inp["u"], inp["w"], inp["rho"], inp["rhow"], flux, inp["adz"])
        return f, flux
    if opts.get("flags"):
        M.set_wm_flags(getattr(M, opts["flags"]))
    if opts.get("force_layout"):
        M.set_plan_layout(opts["layout"])
    p = M.Plan(ncrms, nx, nz, ntr, dtype=dt)
    try:
        if "layout" in opts:
            assert p.layout == opts["layout"]
        if kind == "run_uw":
            # uploaded with OTHER velocities: the step must read the fresh reference-layout u, w it is given
            other = oracle.make_inputs(ncrms, nx, nz, seed=977, dist=oracle.DIST_CONDITIONED, dtype=dt)
            p.upload(inp["f"], other["u"], other["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
            du, dw = to_dev(inp["u"]), to_dev(inp["w"])
            if opts["misalign"]:   # bases at 8 modulo 16: the library converts u, w first
                ub = torch.empty(du.numel() + 1, dtype=du.dtype, device=du.device)
                wb = torch.empty(dw.numel() + 1, dtype=dw.dtype, device=dw.device)
                du = ub[1:].view(du.shape).copy_(du)
                dw = wb[1:].view(dw.shape).copy_(dw)
                assert du.data_ptr() % 16 == 8
            p.run_uw(du, dw)
        else:
            p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])
            if kind == "periodic":
                p.set_boundary(M.BOUNDARY_PERIODIC)
            for _ in range(PERIODIC_STEPS if kind == "periodic" else 1):
                p.run()
        p.sync()
        f, flux = _host_out(inp)
        p.download(f, flux)
    finally:
        p.close()
    return f, flux


def assert_bitwise_but_zero_sign(f, f_ref):
    """EXACT f on signed-zero inputs, the one named exception to the bit-pattern bar: the kernels' max / min (the
    limiter's extrema, the upwind selects pp / pn, the final max(0, .) of :634) are the hardware maximum and minimum,
    which order -0 below +0, where the reference's MAX / MIN (the oracle's `a > b ? a : b`) return the second argument
    when the two compare equal.  A zero can therefore come out with the other sign, and only that: every bit mismatch
    of f is a (+0, -0) pair, the values are equal, and flux stays bit-identical (checked by the caller)."""
    bad = bit_mismatches(f, f_ref)
    if len(bad[0]):
        a, b = f[bad], f_ref[bad]
        assert np.all(a == 0) and np.all(b == 0), \
            f"f: {np.count_nonzero((a != 0) | (b != 0))} of {len(a)} mismatches are not (+0, -0) pairs"


def _tracers(a, ntr):
    return [np.asfortranarray(a[..., t]) for t in range(ntr)] if ntr > 1 else [a]


def check_fast(oracle, R, regime, dt, inp, f, flux, f_ref, flux_ref, ntr, steps, hi):
    """the scale-relative FAST bars (module docstring); returns the worst ratios"""
    u = UNIT[dt]
    worst = [0.0, 0.0, 0.0]
    his = _tracers(hi[0], ntr) if hi is not None else [None] * ntr
    for t, (fi, ft, flt, fr, flr, fh) in enumerate(zip(_tracers(inp["f"], ntr), _tracers(f, ntr), _tracers(flux, ntr),
                                                      _tracers(f_ref, ntr), _tracers(flux_ref, ntr), his)):
        S = float(np.max(np.abs(fi.astype(np.float64))))
        assert S > 0, (regime, t)
        df = float(np.max(np.abs(ft.astype(np.float64) - fr)))
        worst[0] = max(worst[0], df / (steps * u * S))
        assert df <= steps * C_FAST * u * S, \
            f"tracer {t}: max|df| = {df:.3e} = {df / (u * S):.1f} u * max|f_in| (bound {steps * C_FAST:g})"
        nzm = flt.shape[1] - 1
        SF = float(np.max(np.abs(flr[:, :nzm].astype(np.float64))))
        dfl = float(np.max(np.abs(flt[:, :nzm].astype(np.float64) - flr[:, :nzm])))
        if SF > 0:
            worst[1] = max(worst[1], dfl / (steps * u * SF))
        assert dfl <= steps * C_FAST * u * SF, \
            f"tracer {t}: max|dflux| = {dfl:.3e}, max|flux| = {SF:.3e} (bound {steps * C_FAST:g} u)"
        assert_bitwise(flt[:, nzm], flr[:, nzm], f"tracer {t} flux(:, nz)")
        if fh is not None:   # fp32: against the fp64 oracle on the same (fp32) inputs
            e_fast = float(np.max(np.abs(ft.astype(np.float64) - fh)))
            e_ref = float(np.max(np.abs(fr.astype(np.float64) - fh)))
            worst[2] = max(worst[2], e_fast / (2 * e_ref + 4 * u * S))
            assert e_fast <= 2 * e_ref + 4 * u * S, \
                f"tracer {t}: |f_fast32 - f64| = {e_fast:.3e} > 2 * {e_ref:.3e} + 4 u32 * {S:.3e}"
    return worst


@pytest.mark.parametrize("variant", ["exact", "fast"])
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_path_on_every_regime(M, oracle, R, path, variant):
    """One kernel path, one variant, every regime of its dtype; all regimes are run, the failures reported together."""
    name, dt, shape, ntr, kind, opts = path
    var = M.VARIANT_EXACT if variant == "exact" else M.VARIANT_FAST
    periodic = kind == "periodic"
    steps = PERIODIC_STEPS if periodic else 1
    failures = []
    for regime in R.regimes_for(dt):
        M.set_variant(var)
        inp = inputs(R, regime, dt, shape, ntr)
        f_ref, flux_ref = reference(oracle, (regime, np.dtype(dt).name, shape, ntr, periodic), inp, periodic)
        try:
            f, flux = run_path(M, oracle, kind, opts, inp, ntr)
            assert f.dtype == dt and flux.dtype == dt
            if var == M.VARIANT_EXACT:
                errs = []
                for what, a, b in (("f", f, f_ref), ("flux", flux, flux_ref)):
                    try:
                        if regime == "signed_zero" and what == "f":
                            assert_bitwise_but_zero_sign(a, b)
                        else:
                            assert_bitwise(a, b, what)
                    except AssertionError as e:
                        errs.append(str(e))
                assert not errs, "; ".join(errs)
            else:
                hi = None
                if dt == np.float32:
                    inp64 = {k: np.asfortranarray(v.astype(np.float64)) for k, v in inp.items()}
                    hi = reference(oracle, (regime, "f32->f64", shape, ntr, periodic), inp64, periodic)
                w = check_fast(oracle, R, regime, dt, inp, f, flux, f_ref, flux_ref, ntr, steps, hi)
                key = (np.dtype(dt).name, regime)
                old = FAST_WORST.get(key, [(0.0, "")] * 3)
                FAST_WORST[key] = [o if o[0] >= x else (x, name) for o, x in zip(old, w)]
        except AssertionError as e:
            failures.append(f"[{regime}] {e}")
        finally:
            M.set_tile(-1)
            M.set_wm_flags(0)
            M.set_plan_layout(M.LAYOUT_WAVEMAJOR)
    assert not failures, f"{name} {variant}:\n" + "\n".join(failures)


def test_report_fast_ratios():
    """(runs last in this module) the worst FAST ratios per dtype and regime, printed for the record: max|df| / (u S),
    max|dflux| / (u max|flux|) -- per step: divided by the step count for the periodic path -- and for fp32 |f - f64| / (2 |f_oracle32 - f64| + 4 u S)"""
    for (dt, regime), (rf, rfl, rhi) in sorted(FAST_WORST.items()):
        print(f"FAST {dt:8s} {regime:12s} f {rf[0]:7.2f} u*S ({rf[1]})   flux {rfl[0]:7.2f} u*S ({rfl[1]})   "
              f"vs-f64 {rhi[0]:5.3f} ({rhi[1]})")
