"""GPU tests: fp32 with an odd ncrms on the packed kernels (include/mpdata_hip.h section 3f) -- wave-major plans of
(ncrms + 1) / 2 instance pairs whose last pair has a phantom upper half, every plan call, the device and the host call,
against the fp32 CPU oracle on the ODD problem.

Bars (those of tests/test_plan_tall_columns.py, whose `check` is used):
  * EXACT: f (every element, halo columns included) and flux (all nz levels) equal the oracle bit pattern for bit pattern.
  * FAST: per tracer max|f - f_oracle| <= K * 64 u * max|f_in| and the same on flux(:, 1:nzm) against max|flux_oracle|,
    u = 2^-24, K the number of steps; flux(:, nz) bit for bit.
Every test runs with the switch on through mpdata_set_f32_odd_ncrms, which the library did not have before, and on
shapes that were MPDATA_EUNSUPPORTED or reference-layout plans before."""
import numpy as np
import pytest

from plan_harness import reset_defaults, upload
from test_plan_tall_columns import check, download, make, oracle_steps, w_of
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = 0x7FC0DEAD   # a quiet NaN with a payload: the guard bands
GUARD = 67            # reals on either side (odd: the far guard starts off a pair boundary too)


@pytest.fixture(scope="module")
def M(mpdata):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    return mpdata


@pytest.fixture(autouse=True)
def _odd(mpdata):
    """the switch on for the test; the library's defaults before and after"""
    reset_defaults(mpdata)
    mpdata.set_f32_odd_ncrms(1)
    yield
    reset_defaults(mpdata)


VARIANTS = ["exact", "fast"]


def var_of(M, name):
    v = M.VARIANT_EXACT if name == "exact" else M.VARIANT_FAST
    M.set_variant(v)
    return v


def _sid(s):
    return "x".join(str(x) for x in s)


def new_plan(M, shape, T=1):
    p = M.Plan(*shape, T, dtype=F32)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    return p


# (ncrms, nx, nz).  A tile holds 8 / 4 / 2 / 1 pairs at nz <= 8 / 16 / 32 / 64: ncrms = 15, 17 / 7, 9 / 3, 5 / 1, 3 are
# the tile boundaries -1 and +1 there, ncrms = 1 is one pair with a phantom; 31 .. 129: several tiles and more than one
# workgroup of the conversion kernels.  nz: every LPS and its edges.  nx = 70: the park array of EXACT plans.
SHAPES = [
    (1, 5, 3), (3, 1, 8), (15, 5, 8), (17, 37, 8), (129, 5, 3),          # LPS 8
    (5, 5, 9), (7, 37, 16), (9, 5, 16), (63, 1, 9), (65, 5, 16),         # LPS 16
    (3, 5, 17), (5, 70, 28), (7, 5, 32), (31, 5, 28), (33, 37, 17),      # LPS 32
    (1, 5, 33), (3, 37, 58), (9, 70, 64), (15, 5, 58), (17, 1, 64), (129, 5, 33),   # LPS 64
]
# above 64 levels: several waves per instance; 72, 74 / 75, 90: a tail wave of 16 / 32 lanes that holds the last
# windows of 4 / 2 pairs; 65, 91, 128, 238: whole-wave windows (2, 2, 3, 4 of them)
SHAPES_KS = [(1, 5, 65), (3, 5, 72), (5, 1, 74), (7, 5, 75), (9, 5, 90), (3, 37, 91), (5, 5, 128), (1, 5, 238), (3, 70, 72),
             (9, 1, 72), (7, 5, 238)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES + SHAPES_KS, ids=_sid)
def test_one_run(M, oracle, shape, variant):
    """host upload, run, host download"""
    v = var_of(M, variant)
    for dist in (oracle.DIST_CONDITIONED, oracle.DIST_RAW_SIGNED)[:2 if v == M.VARIANT_EXACT else 1]:
        inp = make(oracle, shape, dtype=F32, dist=dist)
        p = new_plan(M, shape)
        try:
            upload(p, inp)
            p.run()
            p.sync()
            assert p.last_kernel_ms() > 0
            f, flux = download(p, inp)
        finally:
            p.close()
        check(M, v, inp, f, flux, *oracle.advect(inp), what=f"{_sid(shape)} dist {dist}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(7, 5, 28), (5, 5, 72), (9, 70, 16)], ids=_sid)
def test_three_tracers_in_sub_ranges(M, oracle, shape, variant):
    v = var_of(M, variant)
    inp = make(oracle, shape, T=3, dtype=F32)
    p = new_plan(M, shape, 3)
    try:
        upload(p, inp)
        p.run(2, 1)
        p.run(0, 2)
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle.advect(inp), what=_sid(shape))


@pytest.mark.parametrize("periodic", [False, True], ids=["given", "periodic"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(9, 37, 8), (5, 5, 28), (3, 5, 72)], ids=_sid)
def test_three_runs(M, oracle, shape, variant, periodic):
    v = var_of(M, variant)
    inp = make(oracle, shape, dtype=F32)
    p = new_plan(M, shape)
    try:
        upload(p, inp)
        if periodic:
            p.set_boundary(M.BOUNDARY_PERIODIC)
        for _ in range(3):
            p.run()
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, 3, periodic), steps=3, what=_sid(shape))


@pytest.mark.parametrize("shape", [(7, 5, 28), (3, 5, 58), (5, 5, 72)], ids=_sid)
def test_run_uw(M, oracle, shape):
    """fresh device velocities through the converting path; the plan holds none afterwards"""
    inp = make(oracle, shape, dtype=F32)
    other = make(oracle, shape, dtype=F32, seed=777)
    p = new_plan(M, shape)
    try:
        upload(p, dict(inp, u=other["u"], w=other["w"]))
        du, dw = to_dev(inp["u"]), to_dev(inp["w"])
        p.run_uw(du, dw)
        p.sync()
        f, flux = download(p, inp)
        with pytest.raises(M.MpdataError) as e:
            p.run()
        assert e.value.code == M.ESTATE
    finally:
        p.close()
    check(M, M.VARIANT_EXACT, inp, f, flux, *oracle.advect(inp), what=_sid(shape))


def cut(a, sl0, n):
    return np.asfortranarray(a[sl0:sl0 + n])


def block_ranges(n):
    """the last instance, the last three, an interior range that starts and ends inside pairs"""
    return [(n - 1, 1), (n - 3, 3), (1, 2)]


BLOCK_SHAPES = [(9, 5, 16), (7, 5, 28), (5, 37, 58), (5, 5, 72)]


@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=_sid)
def test_block_import_then_run(M, oracle, shape):
    """import_block of f, u, w, rho: the plan then behaves as if the arrays with the slice replaced had been imported.
    The phantom is a copy of the plan's last instance, so a block that ends there must refresh it; what a stale one
    would spoil is not visible from outside, the last block is exported on its own all the same."""
    import torch
    n = shape[0]
    A, B = make(oracle, shape, dtype=F32), make(oracle, shape, dtype=F32, seed=4242)
    keys = ("f", "u", "w", "rho")
    for sl0, m in block_ranges(n):
        mix = {k: np.array(v, order="F") for k, v in A.items()}
        for k in keys:
            mix[k][sl0:sl0 + m] = B[k][sl0:sl0 + m]
        f_ref, flux_ref = oracle.advect(mix)
        p = new_plan(M, shape)
        try:
            upload(p, A)
            blk = {k: to_dev(cut(B[k], sl0, m)) for k in keys}   # (alive until the plan's stream is drained)
            p.import_block(sl0, **blk)
            p.run()
            df, dl = to_dev(A["f"]), to_dev(A["flux"])
            p.export_device(f=df, flux=dl)
            bf, bl = to_dev(cut(A["f"], n - 1, 1)), to_dev(cut(A["flux"], n - 1, 1))
            p.export_block(n - 1, f=bf, flux=bl)
            p.sync()
            torch.cuda.synchronize()
        finally:
            p.close()
        what = f"{_sid(shape)} block [{sl0}, {sl0 + m})"
        assert_bitwise(to_host(df), f_ref, what + " f")
        assert_bitwise(to_host(dl), flux_ref, what + " flux")
        assert_bitwise(to_host(bf), cut(f_ref, n - 1, 1), what + " f of the last instance")
        assert_bitwise(to_host(bl), cut(flux_ref, n - 1, 1), what + " flux of the last instance")


@pytest.mark.parametrize("shape", BLOCK_SHAPES, ids=_sid)
def test_block_round_trip(M, oracle, shape):
    """export_block and download_block are slices of the whole export"""
    import torch
    n = shape[0]
    inp = make(oracle, shape, dtype=F32)
    f_ref, flux_ref = oracle.advect(inp)
    p = new_plan(M, shape)
    try:
        upload(p, inp)
        p.run()
        df, dl = to_dev(inp["f"]), to_dev(inp["flux"])
        p.export_device(f=df, flux=dl)
        p.sync()
        torch.cuda.synchronize()
        f, flux = to_host(df), to_host(dl)
        assert_bitwise(f, f_ref, "whole export f")
        assert_bitwise(flux, flux_ref, "whole export flux")
        for sl0, m in block_ranges(n) + [(0, n)]:
            bf, bl = to_dev(np.zeros_like(cut(f, sl0, m))), to_dev(np.zeros_like(cut(flux, sl0, m)))
            p.export_block(sl0, f=bf, flux=bl)
            p.sync()
            torch.cuda.synchronize()
            hf, hl = np.zeros_like(cut(f, sl0, m)), np.zeros_like(cut(flux, sl0, m))
            p.download_block(sl0, hf, hl)
            what = f"{_sid(shape)} block [{sl0}, {sl0 + m})"
            assert_bitwise(to_host(bf), cut(f, sl0, m), what + " export_block f")
            assert_bitwise(to_host(bl), cut(flux, sl0, m), what + " export_block flux")
            assert_bitwise(hf, cut(f, sl0, m), what + " download_block f")
            assert_bitwise(hl, cut(flux, sl0, m), what + " download_block flux")
    finally:
        p.close()


class Guarded:
    """a caller array inside a larger poisoned buffer; off = 1: the array starts 4 bytes off an 8-byte boundary"""

    def __init__(self, a, off):
        import torch
        self.n = a.size
        self.lo = GUARD + 1 + off   # (GUARD + 1 is even and the allocation is aligned far beyond 8 bytes)
        self.buf = torch.from_numpy(np.full(self.lo + self.n + GUARD, POISON, np.uint32).view(np.int32)).to("cuda:0")
        self.t = self.buf[self.lo:self.lo + self.n].view(torch.float32).view(tuple(reversed(a.shape)))
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
        assert self.t.data_ptr() % 8 == 4 * off and self.t.is_contiguous()

    def guards_intact(self):
        g = self.buf.cpu().numpy().view(np.uint32)
        return bool(np.all(g[:self.lo] == POISON) and np.all(g[self.lo + self.n:] == POISON))


INPUTS = ("u", "w", "rho", "rhow", "adz")


def guarded_set(inp, off):
    # the seven arrays take turns: with off = 1 every other one sits on an odd real
    return {k: Guarded(v, (i + off) % 2 if off else 0) for i, (k, v) in enumerate(inp.items())}


def assert_untouched(g, inp, what):
    for k, a in g.items():
        assert a.guards_intact(), f"{what}: the guard band of {k} was written"
    for k in INPUTS:
        assert_bitwise(to_host(g[k].t), inp[k], f"{what}: input {k}")


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-byte"])
@pytest.mark.parametrize("shape", [(1, 5, 3), (9, 5, 16), (7, 37, 28), (65, 5, 16), (3, 5, 58), (5, 5, 72)], ids=_sid)
def test_guard_bands_plan(M, oracle, shape, off):
    """import_device / run / export_device on arrays that end where their allocation could: nothing outside them is
    written, the inputs are not written at all, and the result is that of arrays at any other place"""
    import torch
    inp = make(oracle, shape, dtype=F32)
    f_ref, flux_ref = oracle.advect(inp)
    g = guarded_set(inp, off)
    p = new_plan(M, shape)
    try:
        p.import_device(**{k: a.t for k, a in g.items()})
        p.run()
        p.export_device(f=g["f"].t, flux=g["flux"].t)
        p.sync()
        torch.cuda.synchronize()
    finally:
        p.close()
    assert_untouched(g, inp, _sid(shape))
    assert_bitwise(to_host(g["f"].t), f_ref, "f")
    assert_bitwise(to_host(g["flux"].t), flux_ref, "flux")


CALL_SHAPES = [(5, 5, 33), (7, 37, 58), (3, 5, 64), (9, 5, 72)]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-byte"])
@pytest.mark.parametrize("shape", CALL_SHAPES, ids=_sid)
def test_guard_bands_device_call(M, oracle, shape, off):
    import torch
    inp = make(oracle, shape, dtype=F32)
    f_ref, flux_ref = oracle.advect(inp)
    g = guarded_set(inp, off)
    M.advect_scalar2D(g["f"].t, g["u"].t, g["w"].t, g["rho"].t, g["rhow"].t, g["flux"].t, g["adz"].t)
    torch.cuda.synchronize()
    M.release_host_buffers()
    assert_untouched(g, inp, _sid(shape))
    assert_bitwise(to_host(g["f"].t), f_ref, "f")
    assert_bitwise(to_host(g["flux"].t), flux_ref, "flux")


def device_call(M, inp, stream=None):
    import torch
    d = {k: to_dev(v) for k, v in inp.items()}
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    M.advect_scalar2D(d["f"], d["u"], d["w"], d["rho"], d["rhow"], d["flux"], d["adz"], stream=stream)
    (stream or torch.cuda.current_stream()).synchronize()
    return to_host(d["f"]), to_host(d["flux"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", CALL_SHAPES, ids=_sid)
def test_device_and_host_call(M, oracle, shape, variant):
    v = var_of(M, variant)
    inp = make(oracle, shape, dtype=F32)
    f_ref, flux_ref = oracle.advect(inp)
    try:
        f, flux = device_call(M, inp)
        check(M, v, inp, f, flux, f_ref, flux_ref, what=_sid(shape) + " device call")
        f, flux = np.array(inp["f"], order="F"), np.array(inp["flux"], order="F")
        M.advect_scalar2D_host(f, inp["u"], inp["w"], inp["rho"], inp["rhow"], flux, inp["adz"])
        check(M, v, inp, f, flux, f_ref, flux_ref, what=_sid(shape) + " host call")
    finally:
        M.release_host_buffers()


def test_consecutive_device_calls_and_a_second_stream(M, oracle):
    """the staged plan is kept per thread and shape: two shapes in turn, then the first one again on another stream"""
    import torch
    a, b = make(oracle, (5, 5, 33), dtype=F32), make(oracle, (7, 9, 58), dtype=F32, seed=5)
    ra, rb = oracle.advect(a), oracle.advect(b)
    try:
        for inp, ref in ((a, ra), (b, rb), (a, ra)):
            check(M, M.VARIANT_EXACT, inp, *device_call(M, inp), *ref, what="default stream")
        check(M, M.VARIANT_EXACT, a, *device_call(M, a, torch.cuda.Stream()), *ra, what="second stream")
        check(M, M.VARIANT_EXACT, a, *device_call(M, a), *ra, what="back on the default stream")
    finally:
        M.release_host_buffers()


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(3, 5, 239), (5, 3, 300)], ids=_sid)
def test_tall_columns(M, oracle, shape, variant, steps):
    """with section 3e on as well: ncrms * W = 3 * 5 pseudo-instances (odd: the inner plan has the phantom) and 5 * 6"""
    v = var_of(M, variant)
    M.set_tall_columns(1)
    inp = make(oracle, shape, dtype=F32)
    p = new_plan(M, shape)
    try:
        assert p.level_windows == w_of(shape[2])
        upload(p, inp)
        for _ in range(steps):
            p.run()
        p.sync()
        f, flux = download(p, inp)
    finally:
        p.close()
    check(M, v, inp, f, flux, *oracle_steps(oracle, inp, steps), steps=steps, what=_sid(shape))


def test_tall_device_call(M, oracle):
    M.set_tall_columns(1)
    inp = make(oracle, (3, 5, 239), dtype=F32)
    try:
        check(M, M.VARIANT_EXACT, inp, *device_call(M, inp), *oracle.advect(inp), what="3x5x239 device call")
    finally:
        M.release_host_buffers()


def test_switch_off_in_the_same_process(M):
    """off again, the library is the one it was: no kernel above 32 levels, a reference-layout plan below"""
    assert M.set_f32_odd_ncrms(0) == 1
    with pytest.raises(M.MpdataError) as e:
        M.Plan(9, 6, 33, dtype=F32)
    assert e.value.code == M.EUNSUPPORTED == -2
    p = M.Plan(9, 6, 16, dtype=F32)
    try:
        assert p.layout == M.LAYOUT_REFERENCE
    finally:
        p.close()
    assert M.set_f32_odd_ncrms(1) == 0
    p = M.Plan(9, 6, 33, dtype=F32)
    try:
        assert p.layout == M.LAYOUT_WAVEMAJOR
    finally:
        p.close()
    for lay in (M.LAYOUT_REFERENCE,):   # a forced reference layout keeps its meaning and its error
        M.set_plan_layout(lay)
        with pytest.raises(M.MpdataError) as e:
            M.Plan(9, 6, 33, dtype=F32)
        assert e.value.code == M.EUNSUPPORTED
        p = M.Plan(9, 6, 16, dtype=F32)
        try:
            assert p.layout == M.LAYOUT_REFERENCE
        finally:
            p.close()
