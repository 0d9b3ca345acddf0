"""The model of the level statistics (include/mpdata_hip.h 3g) in plain numpy, and the inputs its tests share.

level_stats(f): for f (ncrms, nx+6, nzm[, T]) in the reference layout, per instance, level and tracer over the interior
columns i = 1 .. nx (array index i + 2): sum = (+0.0 + f_1) + f_2 ... in exactly this order and in f's dtype -- an
explicit loop over i, never np.sum, whose pairwise order is not the defined one --, and the smallest / largest element.
sum_reversed and sum_pairwise are the wrong orders the input guard of tests/test_level_stats_cpu.py measures against.
"""
import numpy as np

from util import bits


def level_stats(f):
    f = np.asarray(f)
    nx = f.shape[1] - 6
    assert nx >= 1
    s = np.zeros(f.shape[:1] + f.shape[2:], f.dtype)          # +0.0
    mn = np.array(f[:, 3], f.dtype)
    mx = np.array(f[:, 3], f.dtype)
    for i in range(1, nx + 1):
        col = f[:, i + 2]
        s = s + col
        mn = np.minimum(mn, col)
        mx = np.maximum(mx, col)
    assert s.dtype == f.dtype
    return np.asfortranarray(s), np.asfortranarray(mn), np.asfortranarray(mx)


def sum_reversed(f):
    nx = f.shape[1] - 6
    s = np.zeros(f.shape[:1] + f.shape[2:], f.dtype)
    for i in range(nx, 0, -1):
        s = s + f[:, i + 2]
    return s


def sum_pairwise(f):
    nx = f.shape[1] - 6
    parts = [np.array(f[:, i + 2]) for i in range(1, nx + 1)]
    while len(parts) > 1:
        parts = [parts[j] + parts[j + 1] if j + 1 < len(parts) else parts[j] for j in range(0, len(parts), 2)]
    return parts[0]


def has_negative_zero(a):
    a = np.asarray(a)
    return bool(np.any((a == 0) & np.signbit(a)))


# ---- inputs.  oracle.make_inputs with dist 3 (raw, mixed magnitudes); interior and halo columns of f are scaled by
# 2**(-(column mod 4)) -- exact, and it makes the rounding of a partial sum depend on what was added before.
def make(oracle, shape, T=1, dtype=np.float64, seed=100):
    """all seven arrays; f (and flux) with T tracers from seeds seed .. seed + T - 1"""
    kw = dict(dist=oracle.DIST_RAW_SIGNED, dtype=dtype)
    inp = oracle.make_inputs(*shape, seed=seed, **kw)
    per = [inp] + [oracle.make_inputs(*shape, seed=seed + t, **kw) for t in range(1, T)]
    scale = (2.0 ** (-1.0 * (np.arange(shape[1] + 6) % 4))).astype(dtype)
    fs = [np.asfortranarray(p["f"] * scale[None, :, None]) for p in per]
    assert all(x.dtype == np.dtype(dtype) for x in fs)
    if T > 1:
        inp["f"] = np.asfortranarray(np.stack(fs, axis=-1))
        inp["flux"] = np.asfortranarray(np.stack([p["flux"] for p in per], axis=-1))
    else:
        inp["f"] = fs[0]
    return inp


# every (shape, tracers, dtype, seed) the GPU tests of tests/test_plan_level_stats.py upload; the seeds are those that pass
# the guard of tests/test_level_stats_cpu.py (it checks the entries with nx >= 3: a sum of one or two terms has one order)
F64, F32 = np.float64, np.float32


def _tile(nz, dtype):
    """instances of one tile of a wave-major plan: 64 / LPS (one above 32 levels), fp32: pairs"""
    lps = 8 if nz <= 8 else 16 if nz <= 16 else 32 if nz <= 32 else 64
    return (64 // lps) * (2 if dtype == F32 else 1)


INPUTS = {}
for _nz in (3, 5, 12, 28, 58, 72, 130):          # fp64: two tiles and one instance of a third
    INPUTS[f"f64-nz{_nz}"] = ((2 * _tile(_nz, F64) + 1, 7, _nz), 1, F64, 100)
for _nx, _seed in ((1, 100), (2, 100), (5, 101), (32, 100)):
    INPUTS[f"f64-nx{_nx}"] = ((5, _nx, 28), 1, F64, _seed)
for _nz in (5, 28, 72):                          # fp32: an even ncrms, and an odd one (a phantom half)
    INPUTS[f"f32-nz{_nz}-even"] = ((2 * _tile(_nz, F32) + 2, 7, _nz), 1, F32, 100)
    INPUTS[f"f32-nz{_nz}-odd"] = ((2 * _tile(_nz, F32) + 1, 7, _nz), 1, F32, 100)
INPUTS.update({
    "f32-nz12-odd-ref": ((9, 7, 12), 1, F32, 100), "f64-nz12-ref": ((9, 7, 12), 3, F64, 100), "f32-nz12-ref": ((10, 7, 12), 1, F32, 100),
    "f64-tall": ((3, 7, 250), 1, F64, 100), "f32-tall-odd": ((3, 7, 250), 1, F32, 100), "f64-tall-kmarch": ((3, 7, 250), 1, F64, 100),
    "f64-blocks": ((11, 7, 28), 3, F64, 100), "f32-blocks": ((11, 7, 28), 3, F32, 100),
    "f64-tall-blocks": ((11, 7, 250), 1, F64, 100), "f32-tall-blocks": ((11, 7, 250), 1, F32, 100),
    "f64-array": ((7, 5, 6), 2, F64, 107), "f32-array": ((7, 5, 6), 2, F32, 114),
})
