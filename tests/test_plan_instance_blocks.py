"""Blocks of CRM instances of a resident plan (include/mpdata_hip.h 3d): mpdata_plan_import_instances_device,
_export_instances_device, _download_instances[_f32] and their Python face Plan.import_block / export_block /
download_block / shard_plan.

The feature moves bits, so every comparison is np.array_equal.  The references are the CPU oracle (oracle.advect on
the block's inputs alone, or on whole inputs with the slice replaced) and the existing whole-plan export; the new
calls are never compared with themselves.  Shapes: every lanes-per-instance size of the wave-major layout, the
tail-wave and window forms above 64 levels, reference-layout plans (nz > 238, forced, fp32 with an odd ncrms), fp32
wave-major plans (instance pairs); blocks: the first and the last instance, the whole plan, blocks that start and end
inside tiles, odd starts and lengths (split fp32 pairs), the padded last tile."""
import ctypes

import numpy as np
import pytest

from plan_harness import upload
from test_periodic_api import wrap
from util import to_dev, to_host

gpu = pytest.mark.gpu

# (ncrms, nx, nz), tracers, dtype, layout forced, layout expected
CASES = [
    ((70, 9, 7), 1, np.float64, None, 1),       # 8 lanes per instance
    ((37, 5, 16), 3, np.float64, None, 1),      # 16; three tracers: tracer sub-ranges on a wave-major plan
    ((130, 32, 28), 1, np.float64, None, 1),    # 32
    ((48, 32, 58), 1, np.float64, None, 1),     # 64
    ((10, 9, 72), 1, np.float64, None, 1),      # tail wave
    ((6, 5, 130), 1, np.float64, None, 1),      # windows
    ((40, 5, 72), 1, np.float64, None, 1),      # above 64 levels with more instances than one workgroup of the block kernel moves
    ((5, 6, 240), 1, np.float64, None, 0),      # nz > 238: reference layout
    ((37, 9, 12), 3, np.float64, 0, 0),         # MPDATA_LAYOUT_REFERENCE; tracer sub-ranges on a reference-layout plan
    ((38, 9, 28), 1, np.float32, None, 1),      # fp32 wave-major: pairs of instances
    ((12, 7, 80), 3, np.float32, None, 1),
    ((33, 10, 20), 1, np.float32, None, 0),     # fp32, odd ncrms: reference layout
]
# one shape per layout and precision (the checks that run the oracle per block)
ORACLE_CASES = [CASES[2], CASES[7], CASES[8], CASES[10]]
ARRAYS = ("f", "u", "w", "rho", "rhow", "adz", "flux")


def _id(c):
    (n, nx, nz), T, dt, lay, _ = c
    return f"{n}x{nx}x{nz}-T{T}-{np.dtype(dt).name}" + ("-ref" if lay == 0 else "")


def tile_instances(nz, dtype):
    """instances of one tile of a wave-major plan (include/mpdata_hip.h 3: 64 / LPS, one above 64 levels; fp32: pairs)"""
    lps = 8 if nz <= 8 else 16 if nz <= 16 else 32 if nz <= 32 else 64
    return (64 // lps) * (2 if np.dtype(dtype) == np.float32 else 1)


def blocks_of(case):
    """(sl0, n): first instance, last instance, everything, one that starts and ends inside tiles around at least
    one whole tile (where ncrms allows), odd start with an odd length, the instances of the (padded) last tile"""
    (ncrms, _, nz), _, dt, _, _ = case
    ts = tile_instances(nz, dt)
    out = [(0, 1), (ncrms - 1, 1), (0, ncrms)]
    s = max(1, ts // 2)
    out.append((s, min(2 * ts, ncrms - s - 1)))       # ts/2 .. 5 ts/2: tile [ts, 2 ts) whole, both ends inside tiles
    out.append((1, 3) if ncrms < 9 else (3, 5))
    last = (ncrms - 1) // ts * ts
    out.append((last, ncrms - last))
    if last > 0:
        out.append((last - 1, ncrms - last))          # ends inside the last tile, its last instance left alone
    seen, uniq = set(), []
    for b in out:
        assert b[0] >= 0 and b[1] >= 1 and b[0] + b[1] <= ncrms, (case, b)
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


def make(oracle, shape, T, dt, seed, ncrms_global=None, sl0=0):
    """make_inputs with T tracers of f (seeds seed .. seed+T-1) and T different flux arrays"""
    kw = dict(dist=oracle.DIST_CONDITIONED, dtype=dt, ncrms_global=ncrms_global, sl0=sl0)
    inp = oracle.make_inputs(*shape, seed=seed, **kw)
    if T > 1:
        per = [oracle.make_inputs(*shape, seed=seed + t, **kw) for t in range(T)]
        inp["f"] = np.asfortranarray(np.stack([p["f"] for p in per], axis=-1))
        inp["flux"] = np.asfortranarray(np.stack([p["flux"] for p in per], axis=-1))
    return inp


def cut(a, sl0, n):
    return np.asfortranarray(a[sl0:sl0 + n])


def merged(A, B, sl0, n, keys=ARRAYS):
    out = {k: np.array(v, order="F") for k, v in A.items()}
    for k in keys:
        out[k][sl0:sl0 + n] = B[k][sl0:sl0 + n]
    return out


class Settings:
    """variant / default layout for the plans created inside the block; restored afterwards"""

    def __init__(self, M, layout=None):
        self.M, self.layout = M, layout

    def __enter__(self):
        self.pv = self.M.set_variant(self.M.VARIANT_EXACT)
        self.pl = self.M.set_plan_layout(self.layout) if self.layout is not None else None

    def __exit__(self, *a):
        self.M.set_variant(self.pv)
        if self.pl is not None:
            self.M.set_plan_layout(self.pl)


def new_plan(M, case, **kw):
    shape, T, dt, lay, want = case
    with Settings(M, lay):
        p = M.Plan(*shape, T, dtype=dt, **kw)
    if not kw:
        assert p.layout == want
    return p


def whole_export(M, p, case):
    """f, flux of the whole plan through the EXISTING export_device, as Fortran-ordered numpy arrays"""
    import torch
    shape, T, dt, _, _ = case
    sh = M.shapes(*shape, T)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    f = torch.empty(sh["f"], dtype=tdt, device="cuda:0")
    flux = torch.empty(sh["flux"], dtype=tdt, device="cuda:0")
    p.export_device(f=f, flux=flux)
    p.sync()
    return to_host(f), to_host(flux)


def block_export(M, p, case, sl0, n, first=0, ntr=None):
    import torch
    (_, nx, nz), T, dt, _, _ = case
    sh = M.shapes(n, nx, nz, T if ntr is None else ntr)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    f = torch.full(sh["f"], -7.0, dtype=tdt, device="cuda:0")
    flux = torch.full(sh["flux"], -7.0, dtype=tdt, device="cuda:0")
    p.export_block(sl0, f=f, flux=flux, first_tracer=first)
    p.sync()
    return to_host(f), to_host(flux)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), f"{what}: {int(np.sum(a != b))} of {a.size} elements differ"


# ---- 1. export = slice of the whole-plan export
@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_export_is_the_slice(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, _, _ = case
    (ncrms, nx, nz) = shape
    inp = make(oracle, shape, T, dt, 100)
    p = new_plan(M, case)
    upload(p, inp)
    p.run()
    F, FL = whole_export(M, p, case)
    for sl0, n in blocks_of(case):
        f, fl = block_export(M, p, case, sl0, n)
        same(f, cut(F, sl0, n), f"f {sl0, n}")
        same(fl, cut(FL, sl0, n), f"flux {sl0, n}")
        if T > 1:   # tracer sub-ranges: two tracers (4-d), the last one alone (3-d)
            f, fl = block_export(M, p, case, sl0, n, first=1, ntr=2)
            same(f, cut(F, sl0, n)[..., 1:3], f"f {sl0, n} tracers 1..2")
            same(fl, cut(FL, sl0, n)[..., 1:3], f"flux {sl0, n} tracers 1..2")
            f, fl = block_export(M, p, case, sl0, n, first=2, ntr=1)
            same(f, cut(F, sl0, n)[..., 2], f"f {sl0, n} tracer 2")
            same(fl, cut(FL, sl0, n)[..., 2], f"flux {sl0, n} tracer 2")
        hf = np.full(M.host_shapes(n, nx, nz, T)["f"], -7, dtype=dt, order="F")
        hl = np.full(M.host_shapes(n, nx, nz, T)["flux"], -7, dtype=dt, order="F")
        p.download_block(sl0, hf, hl)
        same(hf, cut(F, sl0, n), f"download f {sl0, n}")
        same(hl, cut(FL, sl0, n), f"download flux {sl0, n}")
    # periodic: 3 runs; the blocks are read while the plan's halos are stale (a run leaves first-pass values there),
    # then the whole plan (which refreshes them), then the blocks again
    p.set_boundary(M.BOUNDARY_PERIODIC)
    for _ in range(3):
        p.run()
    got = [block_export(M, p, case, sl0, n) for sl0, n in blocks_of(case)]
    F, FL = whole_export(M, p, case)
    G = np.array(F, order="F")
    wrap(f=G)
    same(F, G, "whole export of a periodic plan is wrapped")
    for (sl0, n), (f, fl) in zip(blocks_of(case), got):
        same(f, cut(F, sl0, n), f"periodic f {sl0, n} (stale halos)")
        same(fl, cut(FL, sl0, n), f"periodic flux {sl0, n}")
        f, fl = block_export(M, p, case, sl0, n)
        same(f, cut(F, sl0, n), f"periodic f {sl0, n}")
        same(fl, cut(FL, sl0, n), f"periodic flux {sl0, n} again")
    p.run()
    sl0, n = blocks_of(case)[3]
    hf = np.empty(M.host_shapes(n, nx, nz, T)["f"], dtype=dt, order="F")
    hl = np.empty(M.host_shapes(n, nx, nz, T)["flux"], dtype=dt, order="F")
    p.download_block(sl0, hf, hl)
    F, FL = whole_export(M, p, case)
    same(hf, cut(F, sl0, n), "periodic download f (stale halos)")
    same(hl, cut(FL, sl0, n), "periodic download flux")
    p.close()


@gpu
def test_headline_size(mpdata):
    """65536 x 32 x 28: blocks far into a plan of many tiles, against the whole-plan export and import (inputs made
    on the device; the oracle checks above cover the arithmetic)."""
    import torch
    M = mpdata
    ncrms, nx, nz = 65536, 32, 28
    sh = M.shapes(ncrms, nx, nz, 1)

    def filled(n, seed, sl0=0):
        shn = M.shapes(n, nx, nz, 1)
        d = {k: torch.empty(shn[k], dtype=torch.float64, device="cuda:0") for k in ARRAYS}
        for k in ARRAYS:
            M.fill_synthetic(d[k], k, seed, 1, ncrms_global=ncrms, sl0=sl0)
        return d
    with Settings(M):
        p = M.Plan(ncrms, nx, nz, 1)
    A = filled(ncrms, 100)
    p.import_device(**A)
    p.run()
    F, FL = torch.empty(sh["f"], dtype=torch.float64, device="cuda:0"), torch.empty(sh["flux"], dtype=torch.float64, device="cuda:0")
    p.export_device(f=F, flux=FL)
    p.sync()
    blocks = ((0, 64), (7, 64), (7, 4096), (30001, 777), (65536 - 4097, 4097), (65535, 1))
    for sl0, n in blocks:
        B = filled(n, 1)
        p.export_block(sl0, f=B["f"], flux=B["flux"])
        p.sync()
        assert torch.equal(B["f"], F[..., sl0:sl0 + n]) and torch.equal(B["flux"], FL[..., sl0:sl0 + n]), (sl0, n)
    # import: all seven arrays of other inputs into every block, then one run == a fresh plan on the merged arrays
    X = {k: v.clone() for k, v in A.items()}
    p.import_device(**A)
    for sl0, n in blocks:
        B = filled(n, 4711, sl0)
        p.import_block(sl0, **B)
        for k in ARRAYS:
            X[k][..., sl0:sl0 + n] = B[k]
    G, GL = torch.empty_like(F), torch.empty_like(FL)
    p.export_device(f=G, flux=GL)
    p.sync()
    assert torch.equal(G, X["f"]) and torch.equal(GL, X["flux"])
    with Settings(M):
        q = M.Plan(ncrms, nx, nz, 1)
    q.import_device(**X)
    p.run()
    q.run()
    p.export_device(f=G, flux=GL)
    q.export_device(f=F, flux=FL)
    p.sync()
    q.sync()
    assert torch.equal(G, F) and torch.equal(GL, FL)
    p.close()
    q.close()


# ---- 2. export = the oracle on the block alone (does not lean on the whole-plan export)
@gpu
@pytest.mark.parametrize("case", ORACLE_CASES, ids=_id)
def test_export_is_the_oracle_on_the_block(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, _, _ = case
    ncrms, nx, nz = shape
    p = new_plan(M, case)
    upload(p, make(oracle, shape, T, dt, 100))
    p.run()
    for sl0, n in blocks_of(case):
        # the block's inputs generated on their own: instances [sl0, sl0+n) of the global problem
        f_ref, fl_ref = oracle.advect(make(oracle, (n, nx, nz), T, dt, 100, ncrms_global=ncrms, sl0=sl0))
        f, fl = block_export(M, p, case, sl0, n)
        same(f, f_ref, f"f {sl0, n}")
        same(fl, fl_ref, f"flux {sl0, n}")
    p.close()


# ---- 3. import = the slice replaced
def _import(p, B, sl0, n, keys, first=0, ntr=None):
    dev = {}
    for k in keys:
        a = cut(B[k], sl0, n)
        if ntr is not None and k in ("f", "flux"):
            a = np.asfortranarray(a[..., first:first + ntr]) if ntr > 1 else np.asfortranarray(a[..., first])
        dev[k] = to_dev(a)
    p.import_block(sl0, first_tracer=first, **dev)


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_import_replaces_the_slice(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, _, _ = case
    A, B = make(oracle, shape, T, dt, 100), make(oracle, shape, T, dt, 4711)
    p = new_plan(M, case)
    for sl0, n in blocks_of(case):
        for keys in (ARRAYS, ("f",), ("u", "w")):
            upload(p, A)
            _import(p, B, sl0, n, keys)
            X = merged(A, B, sl0, n, keys)
            F, FL = whole_export(M, p, case)
            same(F, X["f"], f"f before the run {sl0, n} {keys}")
            same(FL, X["flux"], f"flux before the run {sl0, n} {keys}")
            p.run()
            F, FL = whole_export(M, p, case)
            f_ref, fl_ref = oracle.advect(X)
            same(F, f_ref, f"f after the run {sl0, n} {keys}")
            same(FL, fl_ref, f"flux after the run {sl0, n} {keys}")
        if T > 1:   # f and flux of tracers 1..2 only, then of tracer 2 only
            for first, ntr in ((1, 2), (2, 1)):
                upload(p, A)
                _import(p, B, sl0, n, ("f", "flux"), first, ntr)
                X = {k: np.array(v, order="F") for k, v in A.items()}
                for k in ("f", "flux"):
                    X[k][sl0:sl0 + n, ..., first:first + ntr] = B[k][sl0:sl0 + n, ..., first:first + ntr]
                p.run()
                F, FL = whole_export(M, p, case)
                f_ref, fl_ref = oracle.advect(X)
                same(F, f_ref, f"f {sl0, n} tracers {first, ntr}")
                same(FL, fl_ref, f"flux {sl0, n} tracers {first, ntr}")
    p.close()


# ---- 4. round trip
@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_round_trip(mpdata, oracle, case):
    import torch
    M = mpdata
    shape, T, dt, _, _ = case
    _, nx, nz = shape
    p = new_plan(M, case)
    upload(p, make(oracle, shape, T, dt, 100))
    p.run()
    F, FL = whole_export(M, p, case)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    for sl0, n in blocks_of(case):
        sh = M.shapes(n, nx, nz, T)
        f = torch.empty(sh["f"], dtype=tdt, device="cuda:0")
        fl = torch.empty(sh["flux"], dtype=tdt, device="cuda:0")
        p.export_block(sl0, f=f, flux=fl)
        p.import_block(sl0, f=f, flux=fl)
        G, GL = whole_export(M, p, case)
        same(G, F, f"f {sl0, n}")
        same(GL, FL, f"flux {sl0, n}")
    p.close()


# ---- 5. periodic plans ignore imported halos
@gpu
@pytest.mark.parametrize("case", ORACLE_CASES, ids=_id)
def test_periodic_import_ignores_halos(mpdata, oracle, case):
    M = mpdata
    shape, T, dt, _, _ = case
    nx = shape[1]
    A, B = make(oracle, shape, T, dt, 100), make(oracle, shape, T, dt, 4711)
    B["f"][:, [0, 1, 2, nx + 3, nx + 4, nx + 5]] = 1e6   # the sentinel
    p = new_plan(M, case)
    for sl0, n in blocks_of(case):
        upload(p, A)
        p.set_boundary(M.BOUNDARY_PERIODIC)
        p.run()
        _import(p, B, sl0, n, ("f",))
        p.run()
        F, FL = whole_export(M, p, case)
        p.set_boundary(M.BOUNDARY_GIVEN)
        g = np.array(A["f"], order="F")
        wrap(f=g)
        g, gl = oracle.advect(dict(A, f=g))
        g[sl0:sl0 + n] = B["f"][sl0:sl0 + n]
        wrap(f=g)
        g, gl = oracle.advect(dict(A, f=g, flux=gl))
        wrap(f=g)
        assert not (F == 1e6).any()
        same(F, g, f"f {sl0, n}")
        same(FL, gl, f"flux {sl0, n}")
    p.close()


# ---- 6. guard bands around the block's arrays
@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_export_guard_bands(mpdata, oracle, case):
    import torch
    M = mpdata
    shape, T, dt, _, _ = case
    _, nx, nz = shape
    p = new_plan(M, case)
    upload(p, make(oracle, shape, T, dt, 100))
    p.run()
    F, FL = whole_export(M, p, case)
    tdt = torch.float64 if dt == np.float64 else torch.float32
    pad = 37   # elements: the arrays start at an address that is aligned to a real and to nothing more
    for sl0, n in blocks_of(case):
        sh = M.shapes(n, nx, nz, T)
        bufs = {}
        for k in ("f", "flux"):
            cnt = int(np.prod(sh[k]))
            raw = (torch.arange(cnt + 2 * pad, device="cuda:0") % 251).to(tdt) - 1000.0
            bufs[k] = (raw, raw.clone(), raw[pad:pad + cnt].view(sh[k]))
        p.export_block(sl0, f=bufs["f"][2], flux=bufs["flux"][2])
        p.sync()
        same(to_host(bufs["f"][2]), cut(F, sl0, n), f"f {sl0, n}")
        same(to_host(bufs["flux"][2]), cut(FL, sl0, n), f"flux {sl0, n}")
        for k, (raw, orig, _) in bufs.items():
            assert torch.equal(raw[:pad], orig[:pad]) and torch.equal(raw[-pad:], orig[-pad:]), (k, sl0, n)
    p.close()


# ---- 7. errors
def _code(fn, *a, **kw):
    import codesign_kernels_amd as M
    with pytest.raises(M.MpdataError) as e:
        fn(*a, **kw)
    return e.value.code


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: these checks come before anything looks at the plan or the arrays
    for plan, sl0, n in ((None, 0, 1), (one, 0, 0), (one, 0, -3), (one, -1, 1)):
        assert L.mpdata_plan_import_instances_device(plan, sl0, n, one, one, one, one, one, one, one, 0, 1) == -1
        assert L.mpdata_plan_export_instances_device(plan, sl0, n, one, one, 0, 1) == -1
        assert L.mpdata_plan_download_instances(plan, sl0, n, one, one) == -1
        assert L.mpdata_plan_download_instances_f32(plan, sl0, n, one, one) == -1
        assert L.mpdata_last_error()


@gpu
def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    case = ((40, 9, 12), 2, np.float64, None, 1)
    shape, T, dt, _, _ = case
    ncrms, nx, nz = shape
    inp = make(oracle, shape, T, dt, 100)
    sh = M.shapes(4, nx, nz, T)
    dev = {k: to_dev(cut(inp[k], 0, 4)) for k in ARRAYS}
    assert all(tuple(dev[k].shape) == tuple(sh[k]) for k in ARRAYS)
    p = new_plan(M, case)
    L = M.lib()
    # a fresh plan is not filled block by block
    assert _code(p.import_block, 0, **dev) == M.ESTATE
    assert _code(p.export_block, 0, f=dev["f"]) == M.ESTATE
    upload(p, inp)
    p.import_block(36, **dev)
    # ranges
    assert _code(p.export_block, 37, f=dev["f"]) == M.EINVAL
    assert _code(p.import_block, 37, f=dev["f"]) == M.EINVAL
    assert _code(p.export_block, ncrms, f=dev["f"]) == M.EINVAL
    assert _code(p.export_block, -1, f=dev["f"]) == M.EINVAL
    ptr = ctypes.c_void_p(dev["f"].data_ptr())
    assert L.mpdata_plan_export_instances_device(p._p, 0, 0, ptr, None, 0, T) == M.EINVAL
    assert L.mpdata_plan_export_instances_device(p._p, 0, ncrms + 1, ptr, None, 0, T) == M.EINVAL
    assert b"41" in L.mpdata_last_error()   # the text names the offending values
    # tracer range, all pointers null
    assert _code(p.export_block, 0, f=dev["f"], first_tracer=1) == M.EINVAL
    assert L.mpdata_plan_export_instances_device(p._p, 0, 4, ptr, None, 0, 0) == M.EINVAL
    assert L.mpdata_plan_export_instances_device(p._p, 0, 4, None, None, 0, T) == M.EINVAL
    assert L.mpdata_plan_import_instances_device(p._p, 0, 4, *([None] * 7), 0, T) == M.EINVAL
    assert L.mpdata_plan_download_instances(p._p, 0, 4, None, None) == M.EINVAL
    # precision of the host form
    hf = np.empty(M.host_shapes(4, nx, nz, T)["f"], dtype=np.float32, order="F")
    assert L.mpdata_plan_download_instances_f32(p._p, 0, 4, ctypes.c_void_p(hf.ctypes.data), None) == M.ESTATE
    # velocities: none in the plan after run_uw
    p.run_uw(to_dev(inp["u"]), to_dev(inp["w"]))
    assert _code(p.import_block, 0, u=dev["u"]) == M.ESTATE
    assert _code(p.import_block, 0, w=dev["w"]) == M.ESTATE
    p.import_block(0, f=dev["f"], rho=dev["rho"] + 1)   # the other arrays are still welcome
    p.sync()
    p.close()


@gpu
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    import torch
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)   # (every rank on device 0: the peer-copy transport)
    case = ((70, 9, 12), 1, np.float64, None, 1)
    shape, T, dt, _, _ = case
    _, nx, nz = shape
    p = new_plan(M, case, devices=[0, 0])
    upload(p, make(oracle, shape, T, dt, 100))
    p.run()
    F, FL = whole_export(M, p, case)
    sh = M.shapes(5, nx, nz, T)
    f = torch.empty(sh["f"], dtype=torch.float64, device="cuda:0")
    fl = torch.empty(sh["flux"], dtype=torch.float64, device="cuda:0")
    assert _code(p.export_block, 3, f=f, flux=fl) == M.EUNSUPPORTED
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    assert _code(p.import_block, 3, f=f) == M.EUNSUPPORTED
    hf = np.empty(M.host_shapes(5, nx, nz, T)["f"], order="F")
    assert _code(p.download_block, 3, hf, None) == M.EUNSUPPORTED
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        assert q.dims == (nloc, nx, nz, T) and q.ngpus == 1
        for sl0, n in ((0, 5), (3, 5), (nloc - 5, 5)):   # shard-local
            q.export_block(sl0, f=f, flux=fl)
            q.sync()
            same(to_host(f), cut(F, s0 + sl0, n), f"shard {g} f {sl0, n}")
            same(to_host(fl), cut(FL, s0 + sl0, n), f"shard {g} flux {sl0, n}")
        assert _code(q.export_block, nloc - 4, f=f) == M.EINVAL
        q.close()   # frees nothing
    G, GL = whole_export(M, p, case)
    same(G, F, "the plan after its views were closed")
    p.close()


# ---- 8. the Python layer checks shapes before it calls the library
@gpu
def test_python_layer_checks_shapes(mpdata, oracle, monkeypatch):
    import torch
    M = mpdata
    case = ((40, 9, 12), 1, np.float64, None, 1)
    shape, T, dt, _, _ = case
    _, nx, nz = shape
    p = new_plan(M, case)
    upload(p, make(oracle, shape, T, dt, 100))

    def never(*a):
        raise AssertionError("the library was called")
    for name in ("mpdata_plan_export_instances_device", "mpdata_plan_import_instances_device", "mpdata_plan_download_instances"):
        monkeypatch.setattr(M.lib(), name, never)
    sh = M.shapes(4, nx, nz, 1)
    f = torch.empty(sh["f"], dtype=torch.float64, device="cuda:0")
    bad_cols = torch.empty((nz - 1, nx + 5, 4), dtype=torch.float64, device="cuda:0")
    flux5 = torch.empty((nz, 5), dtype=torch.float64, device="cuda:0")
    for fn, kw in ((p.export_block, dict(f=bad_cols)), (p.export_block, dict(f=f, flux=flux5)),
                   (p.export_block, dict(f=f.to(torch.float32))), (p.export_block, dict()),
                   (p.import_block, dict(f=f, u=f)), (p.import_block, dict(rho=flux5))):
        with pytest.raises(M.MpdataError) as e:
            fn(0, **kw)
        assert e.value.code == -1 and "libmpdata_hip error -1" in str(e.value)
    with pytest.raises(M.MpdataError):
        p.download_block(0, np.empty((4, nx + 5, nz - 1), order="F"), None)
    p.close()
