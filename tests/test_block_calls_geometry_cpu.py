"""CPU-only guard of tests/test_block_calls_geometry.py and tests/test_block_calls_geometry_big.py: for every case of
theirs (tests/block_geometry.py)
  1. the inputs are sharp: the models' results for instance b differ in bits from those for instance b - 256, those of
     row r from row r - 65535, those of a block from the block with its tiles rotated by one, a slab from the slab 2^31
     elements or 2^32 bytes earlier -- so an index that drops a term cannot land on equal data;
  2. the case has the geometry it is there for (more than one thread block, rows beyond gridDim.y's cap, the tile,
     slice, group and column-batch counts), computed from the formulas of csrc/mpdata_wm_walk.h,
     csrc/mpdata_column_path.hip and csrc/mpdata_diffuse.hip as tests/block_geometry.py restates them;
  3. the six models of a case take well under a second of processor time (the slabs of section D: a few seconds)."""
import time

import numpy as np
import pytest

import block_geometry as G
import diffuse_model as DM
import scale_uw_model as SM
from block_geometry import bits

SEED = 700                       # tests/test_block_calls_geometry.py: SEED, + 1 (array forms), + 2 (rows), + 3 (wave-major)


def six(inp, limit=1.0):
    """the results of the six models on the whole of inp, instance axis first, rows (level, tracer) merged last -> dict"""
    t0 = time.process_time()
    tr = G.Truth(inp)
    shape, T, dt = tr.shape, tr.T, tr.dt
    out = dict(tr.stats())
    out.update(tr.courant())
    out["path"], out["mass"] = tr.paths()
    tr.add(G.make_d(shape, T, dt, 300, shape[0]))
    out["f_add"] = tr.f.copy(order="F")
    tr.scale(SM.make_s(shape, dt, 400), SM.make_s(shape, dt, 1400))
    out["u"], out["w"] = tr.u, tr.w
    out["zflux"] = tr.diffuse(DM.make_coeffs(shape[0], shape[1], shape[2], dt, 500))
    out["f_diffuse"] = tr.f
    spent = time.process_time() - t0
    assert spent < limit, f"the six models took {spent:.2f} s"
    return out


def rows_last(a, keep):
    """(n, [columns,] rows): the axes after the first `keep` merged in Fortran order"""
    return a.reshape(a.shape[:keep] + (-1,), order="F")


def differs_along(a, axis, shift, what):
    """every index i >= shift of `axis` holds other bits than index i - shift (in at least one element of the rest)"""
    a = np.moveaxis(bits(a), axis, 0)
    assert a.shape[0] > shift, (what, a.shape, shift)
    ne = (a[shift:] != a[:-shift]).reshape(a.shape[0] - shift, -1).any(axis=1)
    assert ne.all(), f"{what}: index {shift + int(np.argmin(ne))} equals the one {shift} before"


# ---- A
@pytest.mark.parametrize("name", list(G.REF_KINDS))
def test_a_plans_are_sharp_beyond_one_thread_block(name):
    shape, T, dt, sw, blocks = G.REF_KINDS[name]
    assert shape[0] > G.TB and 3 <= shape[1] <= 5 and 5 <= shape[2] <= 12 and T == 2
    if dt == G.F32 and not sw.get("ref"):
        assert shape[0] % 2 == 1                          # an odd fp32 plan without the switch keeps the reference layout
    for k, v in six(G.make_inputs(shape, T, dt, SEED)).items():
        differs_along(v, 0, G.TB, f"{name} {k}")
    if blocks is G.BLOCKS_600:
        ncrms = shape[0]
        res = [(ncrms + s if s < 0 else s, ncrms - max(s, 0) if n is None else n) for s, n in blocks]
        assert res[0] == (0, ncrms) and (ncrms - 1, 1) in res
        for sl0, n in res[1:]:
            assert sl0 + n <= ncrms and n != ncrms                 # the leading dimension differs from n
        assert any(sl0 % G.TB and n > G.TB for sl0, n in res)      # sl0 no multiple of 256, more than one thread block
        # bi and sl0 + bi in different thread blocks
        assert any(sl0 // G.TB == 0 and (sl0 + n - 1) // G.TB > (n - 1) // G.TB for sl0, n in res[1:])


@pytest.mark.parametrize("ncrms,dt", G.ARRAY_A)
def test_a_array_forms_are_sharp(ncrms, dt):
    nx, nz = G.ARRAY_A_SHAPE[ncrms]
    assert ncrms in (257, 300, 600) and ncrms > G.TB and 3 <= nx <= 5 and 5 <= nz <= 12
    for k, v in six(G.make_inputs((ncrms, nx, nz), 2, dt, SEED + 1)).items():
        differs_along(v, 0, G.TB, f"array forms n{ncrms} {k}")


# ---- B
@pytest.mark.parametrize("dt", [G.F64, G.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", list(G.ROW_CASES))
def test_b_rows_wrap_onto_other_data(case, dt):
    (ncrms, nx, nz), T = G.ROW_CASES[case]
    rows = G.rows_of(case)
    assert ncrms == 3 and 1 <= nx <= 3
    assert rows and all(G.YMAX < r <= 66000 for r in rows.values()), rows
    inp = G.make_inputs((ncrms, nx, nz), T, dt, SEED + 2)
    for a in inp.values():
        assert a.nbytes < 50e6
    r = six(inp)
    if case.startswith("f-rows"):
        assert nz - 1 >= 3 and (T >= 2 or nz - 1 > G.YMAX)
        if T > 1:      # the wrapped rows cross a tracer boundary
            assert G.YMAX // (nz - 1) < (rows["stats"] - 1) // (nz - 1) and G.YMAX % (nz - 1) != 0
        check = {k: rows_last(r[k], 1) for k in ("sum", "min", "max")}
        check.update({k: rows_last(r[k], 2) for k in ("f_add", "f_diffuse")})
    elif case == "uw-rows":
        check = {k: r[k] for k in ("clev", "u", "w")}
        assert r["w"].shape[-1] == rows["scale_w"] and r["u"].shape[-1] == rows["scale_u"] == rows["courant"]
    else:
        check = {"path": rows_last(r["path"], 1)}
        if "mass" in rows:
            check["mass"] = r["mass"]
    for k, v in check.items():
        assert v.shape[-1] in rows.values(), (k, v.shape, rows)
        differs_along(v, v.ndim - 1, G.YMAX, f"{case} {k}")


# ---- C
WANT_TILES = {"f64-n601-nx32-nz28": (301, 1), "f32-n601-nx32-nz28-odd": (151, 1), "f32-n1030-nx8-nz6": (65, 1),
              "f64-n300-nx9-nz72": (300, 2), "f64-n130-nx8-nz200": (130, 4)}


@pytest.mark.parametrize("name", list(G.WM_KINDS))
def test_c_blocks_reach_many_tiles_of_other_data(mpdata, name):
    shape, T, dt, sw, blocks = G.WM_KINDS[name]
    ncrms, nx, nz = shape
    W, nz_w = 1, None
    if sw.get("tall"):
        W, _, nz_w, _, _ = mpdata.level_window(nz, 0)
        assert W > 1 and nz > 238 and nz_w <= 64
    geo = lambda sl0, n, ntr: G.wm_geometry(shape, dt, sl0, n, ntr, W, nz_w)
    g = geo(0, ncrms, T)
    spt = g["spt"]
    if name in WANT_TILES:
        assert (g["ntiles"], g["nslice"]) == WANT_TILES[name] and g["ntile"] == g["ntiles"]
    else:
        assert g["ntiles"] == ncrms * W >= 300 and spt == 1
    assert ncrms % spt or spt == 1                      # the last tile is partly padding (or a tile is an instance)
    assert blocks[0] == (0, ncrms, 0, T)
    deep, straddle, last = blocks[1], blocks[2], blocks[3]
    assert geo(*deep[:2], 1)["t0"] >= (100 if g["ntiles"] >= 130 else 50)
    assert geo(*straddle[:2], 1)["ntile"] >= 0.6 * g["ntiles"]
    for sl0, n, _, _ in (deep, straddle):
        assert spt == 1 or (sl0 % spt and (sl0 + n) % spt)            # from mid-tile to mid-tile
        assert dt == G.F64 or (sl0 % 2 and (sl0 + n) % 2)             # fp32: a pair split at both ends
    assert last[:2] == (ncrms - 1, 1)
    if T > 1:
        assert any(ntr == T for _, _, _, ntr in blocks[1:]) and any(ntr < T and first > 0 for _, _, first, ntr in blocks)
    if (nx, nz) == (32, 28):
        cp = G.column_path_geometry(shape, dt, 0, ncrms)
        assert (cp["ncb"], cp["CB"]) == (4, 8) and cp["ngroup"] * cp["ncb"] * T >= 100
        assert g["blocks"] * 4 >= g["waves"] >= 100 * T and G.diffuse_groups(shape, dt, 0, ncrms) * T >= 76
    if name == "f64-n130-nx8-nz200":
        assert G.diffuse_groups(shape, dt, 0, ncrms) == g["ntiles"]   # a workgroup per tile
    # sharp: every instance of a block differs from the one a tile earlier (the block's tiles rotated by one)
    r = six(G.make_inputs(shape, T, dt, SEED + 3))
    per = max(1, spt // W) if W > 1 else spt
    for sl0, n, _, _ in blocks:
        if n > per:
            for k, v in r.items():
                differs_along(np.concatenate([v[sl0:sl0 + n], v[sl0:sl0 + per]]), 0, per, f"{name} block {sl0, n} {k}")


# ---- D
WRAPS = {G.F32: (2 ** 31, 2 ** 30), G.F64: (2 ** 29,)}      # elements: 2^31 elements and 2^32 bytes; fp64: 2^32 bytes


@pytest.mark.parametrize("dt", [G.F32, G.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["f", "u", "w"])
def test_d_a_wrapped_offset_lands_on_another_pattern(kind, dt):
    E = G.slab_elems(kind)
    count = G.BIG_F["tracers"][dt] if kind == "f" else G.BIG_UW["slabs"][dt]
    total = count * E + (G.BIG_UW["ncrms"] * (G.BIG_UW["nx"] + 4) if kind == "w" else 0)
    if dt == G.F32:
        assert total > 2 ** 31 and total * 4 > 2 ** 33
    else:
        assert total * 8 > 2 ** 32 and total < 2 ** 31
    if kind != "f":
        assert count % G.BIG_S == 1          # the top slab is pattern 0 (block_geometry.big_uw_inputs)
    for wrap in WRAPS[dt]:
        assert total > wrap
        hit = 0
        for t in range(count):
            src = G.wrapped_patterns(t, E, wrap)
            assert t % G.BIG_S not in src, (kind, t, wrap, src)
            hit += bool(src)
        assert hit >= 1                      # there are slabs beyond the mark
    assert G.BIG_S >= 3


@pytest.mark.parametrize("dt", [G.F32, G.F64], ids=["f32", "f64"])
def test_d_slabs_differ(dt):
    """every slab differs in bits from every other one in every instance (and row), and the models take seconds at most"""
    inp = G.make_inputs(G.BIG_F["shape"], G.BIG_S, dt, 704)
    r = six(inp, limit=8.0)
    for k in ("sum", "min", "max", "path", "mass", "f_add", "f_diffuse", "zflux"):
        v = bits(r[k])
        for a in range(G.BIG_S):
            for b in range(a):
                ne = v[..., a] != v[..., b]
                assert ne.reshape(ne.shape[0], -1).any(axis=1).all(), (k, a, b)
    sl0, n = G.BIG_F["block"]
    assert 0 < sl0 and sl0 + n < G.BIG_F["shape"][0] and n > G.TB
    # u, w: runs of L levels
    L, S = G.BIG_UW["L"], G.BIG_S
    uw = G.big_uw_inputs(dt, 705)
    t0 = time.process_time()
    tr = G.Truth(uw)
    clev = tr.courant()["clev"]
    tr.scale(SM.make_s(tr.shape, dt, 400), SM.make_s(tr.shape, dt, 400))
    assert time.process_time() - t0 < 8.0
    for k, v in (("clev", clev), ("u", tr.u), ("w", tr.w[..., :-1])):
        v = bits(v).reshape(v.shape[:-1] + (S + 1, L))
        for a in range(S):
            for b in range(a):
                assert (v[..., a, :] != v[..., b, :]).any(), (k, a, b)
        if k != "clev":
            assert np.array_equal(v[..., S, :], v[..., 0, :])        # the top slab is slab 0 again
    # the top slab's clev differs from slab 0's only where w(k + 1) does: at its last level
    c = bits(clev).reshape(clev.shape[0], S + 1, L)
    assert np.array_equal(c[:, S, :-1], c[:, 0, :-1]) and (c[:, S, -1] != c[:, 0, -1]).any()


def test_d_plan_reaches_past_4_gib():
    P = G.BIG_PLAN
    shape, T, S = P["shape"], P["T"], P["S"]
    (sl0, n), (first, ntr) = P["block"], P["tracers"]
    tile_b, tracer_b = G.wm_f_strides(shape)
    g = G.wm_geometry(shape, G.F64, sl0, n, ntr)
    mark = 2 ** 32
    assert T * tracer_b > mark and first + ntr == T and first % S == 0 and ntr == S
    assert (T - 1) * tracer_b > mark                                    # a whole tracer lies beyond the mark ...
    t_mark = mark // tracer_b
    assert first <= t_mark < T - 1
    tile_mark = (mark - t_mark * tracer_b) // tile_b
    assert g["t0"] < tile_mark < g["t1"]                                # ... and the block straddles it in the tracer before
    assert sl0 % g["spt"] and (sl0 + n) % g["spt"] and n > P["period"] and sl0 % P["period"]
    # the byte 2^32 bytes earlier lies in a tracer of another pattern
    d = mark // tracer_b
    assert d % S not in (0, S - 1)
    assert g["ntile"] >= 2000 and G.column_path_geometry(shape, G.F64, sl0, n)["ncb"] == 4
    # sharp: the slab's instances all differ from each other's period neighbours trivially (one period is drawn per element);
    # the patterns differ
    r = six(G.make_inputs((P["period"],) + shape[1:], S, G.F64, 706), limit=4.0)
    for k in ("sum", "path", "mass", "f_add", "f_diffuse", "zflux"):
        v = bits(r[k])
        for a in range(S):
            for b in range(a):
                ne = v[..., a] != v[..., b]
                assert ne.reshape(ne.shape[0], -1).any(axis=1).all(), (k, a, b)
    differs_along(r["clev"], 0, 1, "plan clev")
