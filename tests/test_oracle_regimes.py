"""CPU tests: the oracle on the value regimes of oracle/regimes.py (small magnitudes where the limiter's eps
dominates, large ones, sparse and front-like fields, zero and signed-zero velocities, subnormal fp32).

The fixtures under tests/golden/ (manifest key "regimes") are outputs of the reference program itself, fp64 and
its fp32 build; the bar is the bit pattern (+0.0 and -0.0 differ).  The unit-scale cases of
test_oracle_golden.py cannot see the fp32 eps at all (any eps from 1e-20 to 2e-10 gives the same bits there);
these can."""
import hashlib

import numpy as np
import pytest

from util import assert_bitwise, load_golden, regime_cases

CASES = [(c, np.float64) for c in regime_cases("f64")] + [(c, np.float32) for c in regime_cases("f32")]


def _inputs_sha(inp):
    return hashlib.sha256(b"".join(inp[k].tobytes(order="F")
                                   for k in ("adz", "f", "u", "w", "rho", "rhow", "flux"))).hexdigest()


@pytest.fixture(scope="module")
def regimes(oracle):
    from oracle import regimes as R
    return R


def test_every_regime_has_fixtures_in_both_precisions(regimes):
    for dtype, tag in ((np.float64, "f64"), (np.float32, "f32")):
        have = {c["regime"] for c in regime_cases(tag) if (c["ncrms"], c["nx"], c["nz"]) == (8, 32, 28)}
        assert have == set(regimes.regimes_for(dtype)), tag


@pytest.mark.parametrize("case,dtype", CASES, ids=[c["name"] for c, _ in CASES])
def test_oracle_matches_reference_on_value_regimes_bitwise(oracle, regimes, case, dtype):
    """The oracle (both precisions) against the reference on every regime; when oracle/_ref holds the reference
    binary for the shape it is run as well (as test_reference_binary_still_agrees does for the unit-scale cases)."""
    inp = regimes.make(case["regime"], case["ncrms"], case["nx"], case["nz"], seed=case["seed"], dtype=dtype)
    assert _inputs_sha(inp) == case["inputs_sha256"]          # the inputs regenerate to the fixture's bytes
    f_ref, flux_ref = load_golden(case)
    assert f_ref.dtype == dtype
    assert hashlib.sha256(f_ref.tobytes(order="F")).hexdigest() == case["f_sha256"]
    assert hashlib.sha256(flux_ref.tobytes(order="F")).hexdigest() == case["flux_sha256"]
    f, flux = oracle.advect(inp)
    assert_bitwise(f, f_ref, f"{case['name']} f")
    assert_bitwise(flux, flux_ref, f"{case['name']} flux")
    if oracle.ref_exe(case["ncrms"], case["nx"], case["nz"], dtype) is not None:
        f_bin, flux_bin, _ = oracle.run_reference(inp)
        assert_bitwise(f, f_bin, f"{case['name']} f (reference binary)")
        assert_bitwise(flux, flux_bin, f"{case['name']} flux (reference binary)")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_regimes_are_what_they_claim(regimes, dtype):
    """The generator: deterministic, shapes of make_inputs, and each regime's defining property."""
    R = regimes
    n, nx, nz = 6, 10, 9
    for r in R.regimes_for(dtype):
        a, b = R.make(r, n, nx, nz, seed=3, dtype=dtype), R.make(r, n, nx, nz, seed=3, dtype=dtype)
        assert all(a[k].tobytes(order="F") == b[k].tobytes(order="F") for k in a), r
        assert all(v.dtype == dtype and v.flags["F_CONTIGUOUS"] for v in a.values()), r
        assert all(np.isfinite(v).all() for v in a.values()), r
    s20 = R.make("scaled_m20", n, nx, nz, dtype=dtype)["f"]
    base = R.make("calm", n, nx, nz, dtype=dtype)["f"]
    assert np.array_equal(s20, base * dtype(2.0 ** -20))
    sp = R.make("sparse", 8, 32, 28, dtype=dtype)["f"]
    assert 0.8 < np.mean(sp == 0) < 0.97 and 1e-6 * 0.5 <= sp[sp > 0].min() and sp.max() <= 1e-4
    assert np.any(sp[:, :3] > 0) or np.any(sp[:, -3:] > 0)                     # blobs reach into the halo
    fr = R.make("fronts", n, nx, nz, dtype=dtype)["f"]
    assert set(np.unique(fr)) == {0.0, 1.0}
    calm = R.make("calm", n, nx, nz, dtype=dtype)
    assert np.any(np.all(calm["u"] == 0, axis=(0, 2))) and np.any(np.all(calm["w"] == 0, axis=(0, 1)))
    still = R.make("still", n, nx, nz, dtype=dtype)
    assert not np.any(still["u"]) and not np.any(still["w"])
    sz = R.make("signed_zero", n, nx, nz, dtype=dtype)
    for k in ("f", "u", "w"):
        assert np.any(np.signbit(sz[k]) & (sz[k] == 0)), k
    assert np.any(np.signbit(sz["f"][:, :3]) & (sz["f"][:, :3] == 0))           # in the halo too
    mb = R.make("mixed_batch", n, nx, nz, dtype=dtype, ntracers=3)["f"]
    assert mb.shape == (n, nx + 6, nz - 1, 3)
    assert np.abs(mb[1::2, ..., 0]).max() <= 2.0 ** -30 < np.abs(mb[0::2, ..., 0]).max()
    assert np.abs(mb[..., 1]).max() <= 2.0 ** -30 and np.mean(mb[..., 2] == 0) > 0.5
    if dtype == np.float32:
        tiny = R.make("f32_tiny", n, nx, nz, dtype=dtype)["f"]
        assert tiny.max() < 2.0 ** -120 and np.any((tiny > 0) & (tiny < np.finfo(np.float32).tiny))
    else:
        with pytest.raises(ValueError):
            R.make("f32_tiny", n, nx, nz, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_motion_leaves_the_interior_unchanged_bitwise(oracle, regimes, dtype):
    """Oracle-free property: with u = w = 0 every flux is 0, so interior f (and every tracer of a batch) comes out
    bit for bit as it went in -- on unit-scale, signed-zero-free and sparse fields alike -- and flux(:, 1:nzm) is 0."""
    for shape, ntr in (((8, 32, 28), 1), ((5, 7, 6), 3), ((3, 1, 3), 1)):
        inp = regimes.make("still", *shape, seed=17, dtype=dtype, ntracers=ntr)
        if ntr > 1:
            inp["f"][..., 1] = regimes.make("sparse", *shape, seed=17, dtype=dtype)["f"]
        nx = shape[1]
        f, flux = oracle.advect(inp)
        assert_bitwise(f[:, 3:nx + 3], inp["f"][:, 3:nx + 3], f"{shape} interior f")
        assert not np.any(flux[:, :-1])
        assert_bitwise(flux[:, -1], inp["flux"][:, -1], f"{shape} flux(:, nz)")
