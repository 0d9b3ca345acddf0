"""CPU tests of the level windows of tall columns (include/mpdata_hip.h section 3e): the geometry function of the
library (pure arithmetic: no device), and the proof the design rests on, with the CPU oracle only -- a window of
levels, run as a problem of its own, computes the levels it owns exactly as the tall problem does.

A level is at an ARTIFICIAL edge of a window where the window ends but the column does not.  The margin asked for is 3
real levels: the clamp of kb (below) or www = 0 above the top level spoils the first-pass value of the edge level, the
limiter ratios of the next and the final value of the third.
"""
import numpy as np
import pytest

from util import assert_bitwise


@pytest.fixture(scope="module")
def M(mpdata):
    mpdata.lib()
    return mpdata


def windows(M, nz):
    W = M.level_window(nz, 0)[0]
    out = [M.level_window(nz, h) for h in range(W)]
    assert all(w[0] == W for w in out)
    return out


def test_geometry_for_every_height(M):
    for nz in range(239, 2049):
        nzm = nz - 1
        ws = windows(M, nz)
        W = len(ws)
        assert W == -(-(nzm - 6) // 57), nz   # the fewest windows of at most 63 real levels with 3 + 3 margin levels
        nxt = 1
        for h, (_, k0, nz_w, own0, own1) in enumerate(ws):
            m = nz_w - 1
            assert nz_w <= 64 and nz_w == ws[0][2], (nz, h)          # one height: the windows are instances of ONE plan
            assert k0 >= 0 and k0 + m <= nzm, (nz, h)                 # real levels k0+1 .. k0+m exist
            assert own0 == nxt and own1 >= own0, (nz, h)              # the owned ranges tile 1 .. nzm in order
            nxt = own1 + 1
            assert own0 >= k0 + 1 and own1 <= k0 + m, (nz, h)         # ... inside the window
            if h == 0:
                assert k0 == 0 and own0 == 1, nz                      # the bottom clamp is the real one
            else:
                assert own0 - (k0 + 1) >= 3, (nz, h)                  # 3 real levels above the artificial bottom edge
            if h == W - 1:
                assert k0 + m == nzm and own1 == nzm, nz              # the ghost level is the real level nz
            else:
                assert (k0 + m) - own1 >= 3, (nz, h)                  # 3 real levels below the artificial top edge
        assert nxt == nzm + 1, nz


def test_short_columns_are_one_window_and_bad_arguments(M):
    for nz in (2, 3, 28, 63, 64):
        assert M.level_window(nz, 0) == (1, 0, nz, 1, nz - 1)
    for nz, h in ((64, 1), (64, -1), (300, 6), (300, -1), (239, 5), (1, 0), (0, 0)):
        with pytest.raises(M.MpdataError) as e:
            M.level_window(nz, h)
        assert e.value.code == M.EINVAL
    L = M.lib()
    assert L.mpdata_level_window(300, 2, None, None, None, None) == 6   # any pointer may be NULL
    assert M.level_window(65, 1) == (2, 29, 36, 33, 64)                 # (65 .. 238: the rule holds there too; not used)


# ---- the proof, with the oracle only

LEVEL_AXIS = {"f": 2, "u": 2, "w": 2, "rho": 1, "adz": 1, "rhow": 1, "flux": 1}
GHOST = ("w", "rhow", "flux")   # arrays with nz levels: a window takes its ghost level too


def window_inputs(inp, k0, nz_w):
    out = {}
    for k, a in inp.items():
        n = nz_w if k in GHOST else nz_w - 1
        idx = [slice(None)] * a.ndim
        idx[LEVEL_AXIS[k]] = slice(k0, k0 + n)
        out[k] = np.asfortranarray(a[tuple(idx)])
    return out


def split(M, inp):
    nz = inp["w"].shape[2]
    return [(w, window_inputs(inp, w[1], w[2])) for w in windows(M, nz)]


def merge(parts, f, flux):
    """owned levels of every window's (f, flux) -> the tall arrays (flux level nz is not touched)"""
    for (_, k0, _, own0, own1), (fw, flw) in parts:
        f[:, :, own0 - 1:own1] = fw[:, :, own0 - 1 - k0:own1 - k0]
        flux[:, own0 - 1:own1] = flw[:, own0 - 1 - k0:own1 - k0]
    return f, flux


def seam_refresh(parts):
    """every non-owned level of every window's f := its owner's value, all columns (what the device kernel does)"""
    owner = {}
    for (_, k0, _, own0, own1), (fw, _) in parts:
        for k in range(own0, own1 + 1):
            owner[k] = (fw, k - 1 - k0)
    src = {k: fw[:, :, kk].copy() for k, (fw, kk) in owner.items()}
    for (_, k0, nz_w, own0, own1), (fw, _) in parts:
        for k in range(k0 + 1, k0 + nz_w):
            if not own0 <= k <= own1:
                fw[:, :, k - 1 - k0] = src[k]


def inputs(oracle, kind, shape, dtype):
    if kind == "fronts":
        from oracle import regimes
        return regimes.make("fronts", *shape, seed=100, dtype=dtype)
    return oracle.make_inputs(*shape, seed=100, dist=kind, dtype=dtype)


SHAPES = [(3, 5, 239), (2, 7, 300), (2, 4, 457), (2, 3, 293)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [1, 3, "fronts"], ids=["dist1", "dist3", "fronts"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_windows_compute_their_owned_levels_exactly(M, oracle, shape, kind, dtype):
    inp = inputs(oracle, kind, shape, dtype)
    f_ref, flux_ref = oracle.advect(inp)
    parts = [(w, oracle.advect(wi)) for w, wi in split(M, inp)]
    f, flux = merge(parts, inp["f"].copy(order="F"), inp["flux"].copy(order="F"))
    assert_bitwise(f, f_ref, "f")          # every halo column included
    assert_bitwise(flux, flux_ref, "flux")  # levels 1 .. nzm from the windows, level nz never written


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [1, 3, "fronts"], ids=["dist1", "dist3", "fronts"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_three_steps_with_a_seam_refresh_between_them(M, oracle, shape, kind, dtype):
    inp = inputs(oracle, kind, shape, dtype)
    f_ref, flux_ref = inp["f"], inp["flux"]
    for _ in range(3):
        f_ref, flux_ref = oracle.advect(dict(inp, f=f_ref, flux=flux_ref))
    wins = split(M, inp)
    state = [(w, (wi["f"], wi["flux"])) for w, wi in wins]
    for step in range(3):
        if step:
            seam_refresh(state)
        state = [(w, oracle.advect(dict(wi, f=fw, flux=flw))) for (w, wi), (_, (fw, flw)) in zip(wins, state)]
    f, flux = merge(state, inp["f"].copy(order="F"), inp["flux"].copy(order="F"))
    assert_bitwise(f, f_ref, "f after three steps")
    assert_bitwise(flux, flux_ref, "flux after three steps")


def test_without_the_refresh_the_second_step_is_wrong(M, oracle):
    """the refresh is needed: the margin levels of a window are wrong after a step"""
    inp = inputs(oracle, 1, (2, 4, 300), np.float64)
    f_ref, flux_ref = inp["f"], inp["flux"]
    for _ in range(2):
        f_ref, flux_ref = oracle.advect(dict(inp, f=f_ref, flux=flux_ref))
    wins = split(M, inp)
    state = [(w, (wi["f"], wi["flux"])) for w, wi in wins]
    for step in range(2):
        state = [(w, oracle.advect(dict(wi, f=fw, flux=flw))) for (w, wi), (_, (fw, flw)) in zip(wins, state)]
    f, _ = merge(state, inp["f"].copy(order="F"), inp["flux"].copy(order="F"))
    assert not np.array_equal(f, f_ref)
