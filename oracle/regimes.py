"""oracle/regimes.py -- TEST INFRASTRUCTURE: value regimes of the MPDATA inputs.

make_inputs (oracle.py) draws dense unit-scale fields: f in [0, 1), no exact zeros, no
fronts, no zero velocities, no small magnitudes.  The routine is scale-free except in
one place, the limiter denominators `... + eps` with eps = (real)1.e-10f (reference :509,
:601-612), and it holds branches (max(0, .), min(1, .), the upwind selects) that dense
unit-scale data hardly ever sends one way only.  The regimes below reshape conditioned
inputs so that those places are exercised:

  scaled_m20, scaled_m30   f * 2^-20 / 2^-30: eps-dominated limiter denominators
  scaled_p12               f * 2^12: large magnitudes (absolute bounds fail, relative must not)
  sparse                   f exactly 0 on ~90 % of the cells, halo included; seeded blobs of
                           1e-6 .. 1e-4 (cloud-like): 0 / eps ratios, max(0, .) positivity
  fronts                   f a 0/1 step in x and in k: both limiter clamps active, min(1, .)
                           saturated
  calm                     u exactly 0 on a seeded set of columns, w exactly 0 on a seeded set
                           of levels: the zero-velocity sides of the upwind selects
  still                    u = w = 0 everywhere: interior f must come out unchanged bit for bit
  signed_zero              -0.0 in parts of u, w and of f (halo and interior): the sign of zero
                           through max / min and the pp / pn helpers
  mixed_batch              instances of alternating scale (2^0 beside 2^-30) and, for tracer
                           batches, tracer t drawn from a different regime: cross-tracer and
                           cross-instance leakage of the batched and packed kernel forms
  f32_tiny (fp32 only)     f ~ 2^-120 and below, so the fluxes go subnormal: denormal handling

Everything is numpy and deterministic in (regime, ncrms, nx, nz, seed, dtype[, ntracers]).
The fields are built in fp64 and rounded to the dtype (the scalings are powers of two, so
the fp32 inputs are the fp64 ones rounded, as for make_inputs), except f32_tiny, whose
values only exist as fp32 subnormals and near-subnormals.
"""
import numpy as np

from oracle.oracle import DIST_CONDITIONED, make_inputs, shapes

REGIMES = ("scaled_m20", "scaled_m30", "scaled_p12", "sparse", "fronts", "calm", "still", "signed_zero",
           "mixed_batch", "f32_tiny")
F32_ONLY = ("f32_tiny",)
# regimes that change u and w (the others change f only)
MOVES_VELOCITY = ("calm", "still", "signed_zero")
# tracer t >= 1 of a mixed_batch comes from MIX[(t - 1) % len(MIX)] (tracer 0: alternating instance scales)
MIX = ("scaled_m30", "sparse", "scaled_p12", "fronts")


def regimes_for(dtype):
    """The regimes defined for a dtype."""
    return tuple(r for r in REGIMES if np.dtype(dtype) == np.float32 or r not in F32_ONLY)


def _rng(regime, ncrms, nx, nz, seed, salt=0):
    return np.random.default_rng([int(seed), REGIMES.index(regime), int(ncrms), int(nx), int(nz), int(salt)])


def _sparse_f(base, rng):
    """Zero field with a few boxes (half-widths 1..2 in x and k, centred anywhere incl. the halo)
    per instance; amplitude 10^U(-6, -4) per box, times 0.5 .. 1 from the conditioned field."""
    ncrms, ncol, nzm = base.shape
    f = np.zeros_like(base)
    nblob = max(1, int(round(0.1 * ncol * nzm / 15.0)))
    for sl in range(ncrms):
        for _ in range(nblob):
            ic, kc = int(rng.integers(0, ncol)), int(rng.integers(0, nzm))
            hx, hk = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            amp = 10.0 ** rng.uniform(-6.0, -4.0)
            sx, sk = slice(max(0, ic - hx), ic + hx + 1), slice(max(0, kc - hk), kc + hk + 1)
            f[sl, sx, sk] = amp * (0.5 + 0.5 * base[sl, sx, sk])
    return f


def _fronts_f(shape, rng):
    """Per instance f = 1 where exactly one of (column >= ix, level >= kk) holds, else 0."""
    ncrms, ncol, nzm = shape
    ix = rng.integers(3, ncol - 2, size=ncrms)        # array index of the front column (interior 1..nx)
    kk = rng.integers(0, nzm, size=ncrms) if nzm > 1 else np.zeros(ncrms, np.int64)
    i = np.arange(ncol)[None, :, None]
    k = np.arange(nzm)[None, None, :]
    return ((i >= ix[:, None, None]) != (k >= kk[:, None, None])).astype(np.float64)


def _one_f(regime, inp, ncrms, nx, nz, seed, salt):
    """f (fp64, Fortran order) of one tracer of `regime`, from the conditioned f of that tracer."""
    f = inp["f"]
    if regime == "scaled_m20":
        return f * 2.0 ** -20
    if regime == "scaled_m30":
        return f * 2.0 ** -30
    if regime == "scaled_p12":
        return f * 2.0 ** 12
    if regime == "f32_tiny":
        return f * 2.0 ** -120
    if regime == "sparse":
        return _sparse_f(f, _rng(regime, ncrms, nx, nz, seed, salt))
    if regime == "fronts":
        return _fronts_f(f.shape, _rng(regime, ncrms, nx, nz, seed, salt))
    if regime == "mixed_batch":
        if salt == 0:   # adjacent instances at 2^0 and 2^-30 (the two halves of an fp32 packed pair)
            scale = np.where(np.arange(ncrms) % 2 == 1, 2.0 ** -30, 1.0)
            return f * scale[:, None, None]
        return _one_f(MIX[(salt - 1) % len(MIX)], inp, ncrms, nx, nz, seed, salt)
    if regime == "signed_zero":
        m = _rng(regime, ncrms, nx, nz, seed, 100 + salt).random(f.shape)
        g = f.copy()
        g[m < 0.3] = -0.0
        g[(m >= 0.3) & (m < 0.4)] = 0.0
        return g
    return f   # calm, still: f as conditioned


def make(regime, ncrms, nx, nz, seed=100, dtype=np.float64, ntracers=1):
    """All seven input arrays of `regime` (dict of Fortran-ordered arrays, as make_inputs)."""
    dtype = np.dtype(dtype).type
    if regime not in REGIMES:
        raise ValueError(f"unknown regime {regime!r}")
    if regime in F32_ONLY and dtype != np.float32:
        raise ValueError(f"regime {regime!r} is fp32 only")
    inp = make_inputs(ncrms, nx, nz, seed=seed, dist=DIST_CONDITIONED)
    fs = []
    for t in range(ntracers):
        ft = inp["f"] if t == 0 else make_inputs(ncrms, nx, nz, seed=seed + 1000 * t, dist=DIST_CONDITIONED)["f"]
        fs.append(_one_f(regime, dict(inp, f=ft), ncrms, nx, nz, seed, t))
    u, w = inp["u"].copy(order="F"), inp["w"].copy(order="F")
    if regime == "calm":
        rng = _rng(regime, ncrms, nx, nz, seed, 1)
        u[:, rng.random(u.shape[1]) < 0.35, :] = 0.0
        w[:, :, rng.random(w.shape[2]) < 0.35] = 0.0
    elif regime == "still":
        u[...] = 0.0
        w[...] = 0.0
    elif regime == "signed_zero":
        rng = _rng(regime, ncrms, nx, nz, seed, 2)
        u[rng.random(u.shape) < 0.25] = -0.0
        w[rng.random(w.shape) < 0.25] = -0.0
    out = dict(inp, u=u, w=w)
    if ntracers > 1:
        out["f"] = np.stack(fs, axis=-1)
        out["flux"] = np.stack([inp["flux"]] * ntracers, axis=-1)
    else:
        out["f"] = fs[0]
    sh = shapes(ncrms, nx, nz, ntracers)
    res = {}
    for k, v in out.items():
        assert v.shape == sh[k], (k, v.shape, sh[k])
        res[k] = np.asfortranarray(v.astype(dtype))
    return res
