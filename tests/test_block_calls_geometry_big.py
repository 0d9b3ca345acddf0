"""Section D of tests/test_block_calls_geometry.py: the array forms of the six block calls (include/mpdata_hip.h 3g ..
3l, "64-bit offsets: arrays of 4 GiB and more") on a main array of more than 2^31 elements (fp32, more than 8 GiB) and
of more than 2^32 bytes but fewer than 2^31 elements (fp64).

The big array is never on the host.  A few distinct slabs are built there -- one tracer of f; for u and w, which have no
tracer axis, a run of 64 levels, with rho, adz and w repeating with the same period --, uploaded, and copied device to
device along the slowest axis: slab t holds pattern t % 4 (block_geometry.BIG_S).  The truth is the numpy model on the
slabs.  Small outputs are compared whole on the host, outputs with a row per slab and in-place results slab by slab on
the device (torch.equal of integer views) against uploaded truths.  The slab that holds the element 2^31 elements, or
2^32 bytes, before any element has another pattern (asserted in tests/test_block_calls_geometry_cpu.py), so an offset
that lost its upper bits reads other data.

Each test states its need of device memory; it skips only when torch.cuda.mem_get_info reports less (the message of
tests/test_nlk_edges.py), and frees its tensors before the next one."""
import gc

import numpy as np
import pytest

import block_geometry as G
import courant_model as CM
import diffuse_model as DM
import scale_uw_model as SM
from plan_harness import banded, reset_defaults
from test_block_calls_geometry import bands_ok, same_bits
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
SEED = 704
S = G.BIG_S
DTYPES = pytest.mark.parametrize("dt", [G.F32, G.F64], ids=["f32-above-2^31-elements", "f64-above-2^32-bytes"])


@pytest.fixture(autouse=True)
def _defaults_and_free(mpdata):
    import torch
    reset_defaults(mpdata)
    yield
    reset_defaults(mpdata)
    gc.collect()
    torch.cuda.empty_cache()


def need_memory(gib):
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < gib * 2 ** 30:
        pytest.skip(f"memory shortfall: this case needs {gib} GiB of device memory, torch.cuda.mem_get_info reports "
                    f"{free / 2 ** 30:.1f} GiB free")


def is_big(t, dt):
    """the size section D asks of the main array"""
    if dt == G.F32:
        assert t.numel() > 2 ** 31 and t.numel() * 4 > 2 ** 33
    else:
        assert t.numel() * 8 > 2 ** 32 and t.numel() < 2 ** 31


def assemble(slabs, count, extra=None):
    """slabs (S, ...) on the device -> (count, ...) with slab t = slabs[t % S]; extra: rows appended behind the last slab"""
    import torch
    rows = slabs.shape[1] if extra is not None else None
    if extra is None:
        big = torch.empty((count,) + tuple(slabs.shape[1:]), dtype=slabs.dtype, device=slabs.device)
        for t in range(count):
            big[t].copy_(slabs[t % S])
        return big
    big = torch.empty((count * rows + extra.shape[0],) + tuple(slabs.shape[2:]), dtype=slabs.dtype, device=slabs.device)
    for t in range(count):
        big[t * rows:(t + 1) * rows].copy_(slabs[t % S])
    big[count * rows:].copy_(extra)
    return big


def slabs_equal(big, truth, what, rows=None, last=None):
    """slab t of big (rows: levels per slab of an array without a slab axis) has the bits of truth[t % S] (the last one of
    `last`, if given)"""
    count = big.shape[0] if rows is None else big.shape[0] // rows
    for t in range(count):
        got = big[t] if rows is None else big[t * rows:(t + 1) * rows]
        want = last if (last is not None and t == count - 1) else truth[t % S]
        assert same_bits(got, want), f"{what}: slab {t} (pattern {t % S}) differs"


_F = {}


def f_case(dt):
    """the slabs of f as a problem of S tracers, computed once: (inputs, device slabs of f, rho, adz)"""
    if dt not in _F:
        _F[dt] = G.make_inputs(G.BIG_F["shape"], S, dt, SEED)
    inp = _F[dt]
    return inp, to_dev(inp["f"]), to_dev(inp["rho"]), to_dev(inp["adz"])


def slab_rows(a):
    """a model output (n, ..., S) -> its device form (S, ..., n)"""
    return to_dev(np.asfortranarray(a))


@DTYPES
def test_d_level_stats(mpdata, dt):
    """f of 1800 fp32 / 452 fp64 tracers (8.7 / 4.3 GB), three outputs of a row per tracer.  Needs 14 GiB."""
    import torch
    need_memory(14)
    inp, fs, _, _ = f_case(dt)
    T = G.BIG_F["tracers"][dt]
    ncrms, nx, nz = G.BIG_F["shape"]
    f = assemble(fs, T)
    is_big(f, dt)
    want = G.Truth(inp).stats()
    for k in ("sum", "min", "max"):
        b = banded((T, nz - 1, ncrms), dt)
        torch.cuda.synchronize()
        mpdata.level_stats(f, **{k: b[2]})
        torch.cuda.synchronize()
        bands_ok(b, k)
        slabs_equal(b[2], slab_rows(want[k]), f"level_stats {k}")
        del b
    slabs_equal(f, fs, "level_stats: f afterwards")


@DTYPES
def test_d_column_path(mpdata, dt):
    """the same f; path and mass of a row per tracer.  Needs 12 GiB."""
    import torch
    need_memory(12)
    inp, fs, rho, adz = f_case(dt)
    T = G.BIG_F["tracers"][dt]
    ncrms, nx, nz = G.BIG_F["shape"]
    f = assemble(fs, T)
    is_big(f, dt)
    path, mass = G.Truth(inp).paths()
    sh = mpdata.column_path_shapes(ncrms, nx, T)
    bp, bm = banded(sh["path"], dt), banded(sh["mass"], dt)
    torch.cuda.synchronize()
    mpdata.column_path(f, rho, adz, bp[2], bm[2])
    torch.cuda.synchronize()
    bands_ok(bp, "path")
    bands_ok(bm, "mass")
    slabs_equal(bp[2], slab_rows(path), "column_path: path")
    slabs_equal(bm[2], slab_rows(mass), "column_path: mass")
    slabs_equal(f, fs, "column_path: f afterwards")


@DTYPES
def test_d_level_add(mpdata, dt):
    """the same f, in place; d has a row per tracer and repeats with the slabs.  Needs 12 GiB."""
    import torch
    need_memory(12)
    inp, fs, _, _ = f_case(dt)
    T = G.BIG_F["tracers"][dt]
    ncrms, nx, nz = G.BIG_F["shape"]
    f = assemble(fs, T)
    is_big(f, dt)
    dh = G.make_d(G.BIG_F["shape"], S, dt, 300, ncrms)
    ds = to_dev(dh)
    d = assemble(ds, T)
    mpdata.level_add(f, d)
    torch.cuda.synchronize()
    tr = G.Truth(inp)
    tr.add(dh)
    assert not np.array_equal(tr.f, inp["f"])
    slabs_equal(f, to_dev(tr.f), "level_add: f")
    slabs_equal(d, ds, "level_add: d afterwards")


@DTYPES
def test_d_diffuse(mpdata, dt):
    """the same f, in place, on the block of instances 3 .. 494 (the coefficients have no tracer axis: every tracer takes
    the same ones); the call's own scratch array is another 7.1 / 3.6 GB.  Needs 20 GiB."""
    import torch
    need_memory(20)
    inp, fs, rho, adz = f_case(dt)
    T = G.BIG_F["tracers"][dt]
    ncrms, nx, nz = G.BIG_F["shape"]
    sl0, n = G.BIG_F["block"]
    f = assemble(fs, T)
    is_big(f, dt)
    c = DM.make_coeffs(n, nx, nz, dt, 500)
    dev = {k: to_dev(v) for k, v in c.items()}
    orig = {k: v.clone() for k, v in dev.items()}
    zb = banded((T, nz, n), dt)
    torch.cuda.synchronize()
    mpdata.diffuse(f, rho, adz, dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], zb[2], sl0, n)
    torch.cuda.synchronize()
    for k in dev:
        assert same_bits(dev[k], orig[k]), f"{k} changed"
    bands_ok(zb, "zflux")
    tr = G.Truth(inp)
    zflux = tr.diffuse(c, sl0, n)
    out = np.ones(ncrms, bool)
    out[sl0:sl0 + n] = False
    assert_bitwise(tr.f[out], inp["f"][out], "the model changed an instance outside the block")
    slabs_equal(zb[2], slab_rows(zflux), "diffuse: zflux")
    slabs_equal(f, to_dev(tr.f), "diffuse: f")


_UW = {}


def uw_case(dt):
    """the column of S + 1 slabs of levels the truths of u, w come from (block_geometry.big_uw_inputs), computed once"""
    if dt not in _UW:
        _UW[dt] = G.big_uw_inputs(dt, SEED + 1)
    return _UW[dt]


def level_slabs(a, L):
    """host (n, [columns,] levels) -> device (S + 1, L, [columns,] n): the slabs 0 .. S - 1 and the top slab"""
    t = to_dev(np.asfortranarray(a[..., :(S + 1) * L]))
    return t.view((S + 1, L) + tuple(t.shape[1:]))


def big_uw(inp, dt, which):
    """the big device arrays named in `which`, assembled from the slabs of inp"""
    L, m = G.BIG_UW["L"], G.BIG_UW["slabs"][dt]
    assert m % S == 1 and m > S
    out = {}
    for k in which:
        sl = level_slabs(inp[k], L)
        extra = to_dev(np.asfortranarray(inp["w"][..., (S + 1) * L:])) if k == "w" else None
        out[k] = assemble(sl[:S], m, extra) if extra is not None else assemble(sl[:S], m).view((m * L,) + tuple(sl.shape[2:]))
    return out


@DTYPES
def test_d_courant(mpdata, dt):
    """u and w of 1805 fp32 / 453 fp64 slabs of 64 levels (8.8 + 8.6 GB / 4.4 + 4.3 GB); clev has a row per level.
    Needs 22 GiB."""
    import torch
    need_memory(22)
    inp = uw_case(dt)
    L, m, n = G.BIG_UW["L"], G.BIG_UW["slabs"][dt], G.BIG_UW["ncrms"]
    a = big_uw(inp, dt, ("u", "w", "rho", "adz"))
    is_big(a["u"], dt)
    is_big(a["w"], dt)
    bl, bi = banded((m * L, n), dt), banded((n,), dt)
    torch.cuda.synchronize()
    mpdata.courant(a["u"], a["w"], a["rho"], a["adz"], bl[2], bi[2])
    torch.cuda.synchronize()
    bands_ok(bl, "clev")
    bands_ok(bi, "cinst")
    clev, cinst = CM.courant(inp["u"], inp["w"], inp["rho"], inp["adz"])
    want = level_slabs(clev, L)
    slabs_equal(bl[2], want[:S], "courant: clev", rows=L, last=want[S])
    assert_bitwise(to_host(bi[2]), cinst, "courant: cinst")
    for k in ("u", "w"):
        sl = level_slabs(inp[k], L)
        rows = a[k][:m * L]
        slabs_equal(rows, sl[:S], f"courant: {k} afterwards", rows=L)


@DTYPES
@pytest.mark.parametrize("which", ["u", "w"])
def test_d_scale_uw(mpdata, dt, which):
    """u, or w with its level nz behind the last slab, in place (the other array and its factor are None).  Needs 10 GiB."""
    import torch
    need_memory(10)
    inp = uw_case(dt)
    L, m, n = G.BIG_UW["L"], G.BIG_UW["slabs"][dt], G.BIG_UW["ncrms"]
    a = big_uw(inp, dt, (which,))[which]
    is_big(a, dt)
    s = SM.make_s((n, G.BIG_UW["nx"], 2), dt, 400)
    ds = torch.from_numpy(s).to("cuda:0")
    if which == "u":
        mpdata.scale_uw(a, None, ds, None)
    else:
        mpdata.scale_uw(None, a, None, ds)
    torch.cuda.synchronize()
    assert same_bits(ds, torch.from_numpy(s).to("cuda:0"))
    u, w = SM.scale_uw(inp["u"], inp["w"], s if which == "u" else None, s if which == "w" else None)
    new = u if which == "u" else w
    assert not np.array_equal(new, inp[which])
    want = level_slabs(new, L)
    slabs_equal(a[:m * L], want[:S], f"scale_uw: {which}", rows=L)
    if which == "w":
        assert same_bits(a[m * L:], to_dev(np.asfortranarray(new[..., (S + 1) * L:]))), "scale_uw: level nz of w"


# ---- one wave-major fp64 plan whose f exceeds 2^32 bytes
def test_d_plan_above_4_gib(mpdata):
    """8192 x 32 x 28 with 65 tracers: the plan's f is 4.40 GB (4096 tiles of 16512 bytes per tracer), filled through
    import_device from a device array that repeats five patterns along the tracer axis and 512 instances 16 times along
    the instance axis.  Each of the six calls runs once, on instances 4001 .. 8100 and tracers 60 .. 64: the 2^32-byte
    mark lies in tracer 63 at tile 2063, inside the block.  The truth is the models on the 512 instances, repeated.  The
    plan is a FAST one (nothing here runs it; an EXACT plan may hold a park array of f's size besides).  Needs 14 GiB."""
    import torch
    from test_plan_courant import cour
    from test_plan_column_path import paths
    from test_plan_level_stats import stats
    M = mpdata
    need_memory(14)
    P = G.BIG_PLAN
    shape, T, per, SP = P["shape"], P["T"], P["period"], P["S"]
    (sl0, n), (first, ntr) = P["block"], P["tracers"]
    ncrms, nx, nz = shape
    reps = ncrms // per
    assert reps * per == ncrms and first % SP == 0 and ntr == SP
    inp = G.make_inputs((per, nx, nz), SP, G.F64, SEED + 2)
    tr = G.Truth(inp)
    idx = (sl0 + np.arange(n)) % per                       # the slab instance of every instance of the block
    rep = lambda a: to_dev(a).repeat((1,) * (a.ndim - 1) + (reps,))          # along the instance axis (torch: the last one)
    old = rep(inp["f"])                                    # (SP, nzm, nx + 6, ncrms)
    big = torch.empty((T,) + tuple(old.shape[1:]), dtype=torch.float64, device="cuda:0")
    for t in range(T):
        big[t].copy_(old[t % SP])
    assert big.numel() * 8 > 2 ** 32
    M.set_variant(M.VARIANT_FAST)
    p = M.Plan(*shape, T, dtype=G.F64)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    flux = torch.zeros(M.shapes(*shape, T)["flux"], dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dev = {k: rep(inp[k]) for k in ("u", "w", "rho", "rhow", "adz")}      # (alive until the plan's stream is through with them)
    p.import_device(f=big, flux=flux, **dev)
    p.sync()
    del flux, dev

    def f_is(new, what):
        """the plan's whole f: the block's instances of tracers first .. hold `new` (SP, ..., ncrms), everything else `old`"""
        p.export_device(f=big)
        p.sync()
        for t in range(T):
            want = old[t % SP]
            if t >= first:
                want = want.clone()
                want[..., sl0:sl0 + n] = new[t - first][..., sl0:sl0 + n]
            assert same_bits(big[t], want), f"{what}: tracer {t} differs"

    f_is(old, "after the import")
    # 3g, 3h, 3k
    got, want = stats(p, G.F64, nz - 1, sl0, n, first, ntr), tr.stats()
    for k in want:
        assert_bitwise(got[k], want[k][idx], f"level_stats: {k}")
    got, want = cour(p, G.F64, nz - 1, sl0, n), tr.courant()
    for k in want:
        assert_bitwise(got[k], want[k][idx], f"courant: {k}")
    got, want = paths(M, p, G.F64, nx, sl0, n, first, ntr), tr.paths()
    assert_bitwise(got[0], want[0][idx], "column_path: path")
    assert_bitwise(got[1], want[1][idx], "column_path: mass")
    # 3i
    from test_plan_level_add import add
    from test_plan_scale_uw import scale
    d = G.make_d((per, nx, nz), SP, G.F64, 300, per)
    add(p, np.asfortranarray(d[idx]), sl0, n, 0, first)
    tr.add(d)
    f_is(rep(tr.f), "level_add")
    # 3j: through the Courant number of the whole plan
    before = tr.courant()
    su, sw = SM.make_s((per, nx, nz), G.F64, 400), SM.make_s((per, nx, nz), G.F64, 1400)
    scale(p, np.ascontiguousarray(su[idx]), np.ascontiguousarray(sw[idx]), sl0, n)
    tr.scale(su, sw)
    after = tr.courant()
    got = cour(p, G.F64, nz - 1, 0, ncrms)
    inside = np.zeros(ncrms, bool)
    inside[sl0:sl0 + n] = True
    for k in after:
        want = np.where(inside.reshape((-1,) + (1,) * (after[k].ndim - 1)), np.concatenate([after[k]] * reps), np.concatenate([before[k]] * reps))
        assert not np.array_equal(after[k], before[k])
        assert_bitwise(got[k], np.asfortranarray(want) if want.ndim > 1 else want, f"scale_uw: {k} of the whole plan")
    # 3l
    from test_block_calls_geometry import plan_diffuse
    c = DM.make_coeffs(per, nx, nz, G.F64, 500)
    z = plan_diffuse(p, shape, G.F64, {k: np.asfortranarray(v[idx]) for k, v in c.items()}, sl0, n, first, ntr)
    assert_bitwise(z, tr.diffuse(c)[idx], "diffuse: zflux")
    f_is(rep(tr.f), "diffuse")
    p.close()
