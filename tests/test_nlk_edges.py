"""The flux-gather kernels of libnlk_hip.so where masking and index edges hide errors (the reference loop is
nested_loops/nested.F90:123-157).  tests/test_nlk.py feeds them oracle/nlk.py::make_inputs, whose tracerCur is ZERO
outside every cell's [minLevelCell, maxLevelCell]: a kernel that masked nothing would add 0.0 * wgt * coef and pass
bit for bit.  Here every element the reference never reads holds a fill value (-1e34, +1e300, NaN), the level ranges
and cell counts take their edge values, and the arrays sit at the bases, sizes and offsets where launch() changes
kernel form.

Bars.  EXACT: bit-pattern equality with the oracle on rows 1..nVertLevels; padding rows keep their pre-fill.
FAST (FMA contraction): derived, not measured.  A term (tracer * (ntf*mask)) * (c1 + (c3*coef3rdOrder)*sgn) is
computed with FIVE rounded operations: ntf*mask, tracer*wgt, c3*coef3rdOrder, the addition of c1 (sgn = +-1: that
product is exact) and the last product; every one enters the term as a factor (1 + delta), the two of the coefficient
sum relative to |c1| + |c3*coef3rdOrder|.  The running sum starts from 0.0, so its first addition 0.0 + x is exact:
n terms, n the clipped count, take n - 1 rounded additions, and the first term passes through all of them.  The
longest chain is therefore 5 + (n - 1) = n + 4 roundings, and each evaluation, the oracle's and the kernel's, is
within gamma(n + 4) * S of the exact value, S = sum |tracer| |ntf*mask| (|c1| + |c3*coef3rdOrder|) over the contributing
cells in np.longdouble, gamma(m) = m u / (1 - m u), u = 2^-53.  So |out - ref| <= 2 gamma(n + 4) S; the bound is
homogeneous in every input, so it is scale-free; where S = 0 it demands equality.  FMA contraction only removes
roundings.  (The model has no underflow term; the subnormal normalThicknessFlux values of the scale cases are held to
the same bound.)"""
import os

import numpy as np
import pytest

from util import assert_bitwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (-1, 0, 1, 2)
PREFILL = -3.5
NV_SHAPES = (1, 2, 63, 64, 65, 100, 127, 128, 129, 200)
NADVS = (1, 10, 12, 20, 64, 65, 70)
N_EDGES, N_CELLS = 67, 45                     # >= what make_inputs_edges needs for every class; 67 = 16 workgroups + 3 waves
FAST_WORST = {}                               # regime -> (worst |fast - ref| / (2 gamma S), where)


@pytest.fixture(scope="module")
def N():
    from oracle import nlk
    nlk.build_lib()
    return nlk


def nvldims(nV):
    """nVertLevels itself; the next even number; an odd number above an even nVertLevels (the even-nvldim condition
    of the two-level forms fails); values more than 2 above, one odd and one even"""
    return sorted({nV, nV + 1, nV + 2 - (nV & 1), nV + 5, nV + 6})


# ------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("nV", NV_SHAPES)
def test_generator_produces_every_class(N, nV):
    for nvldim in nvldims(nV):
        for nAdv in NADVS:
            inp = N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, seed=nV + nAdv, nvldim=nvldim)
            cl = N.edge_classes(inp)
            if nV == 1:
                cl.pop("min>max")             # needs 1 <= max < min <= ... two levels; min > nV covers nV = 1
            missing = [k for k, v in cl.items() if not v]
            assert not missing, (nV, nvldim, nAdv, missing)
            assert {"max=0", "max<0", "max>nvldim", "min>nV", "min<=0", "min=max", "count=0", "count<0",
                    f"count={nAdv}", f"count={nAdv + 3}", "count=21"} <= set(cl)
            assert ("nV<max<=nvldim" in cl) == (nvldim > nV)
            assert all((f"max={b}" in cl) == (b <= nV) for b in N.LEVEL_BOUNDARIES)


@pytest.mark.parametrize("fill", [-1e34, 1e300, float("nan")], ids=["mpas-fill", "1e300", "nan"])
@pytest.mark.parametrize("nV,nvldim,nAdv", [(1, 1, 1), (2, 7, 10), (65, 66, 12), (100, 105, 20), (129, 130, 65), (200, 200, 70)])
def test_poison_sits_only_where_the_reference_never_reads(N, nV, nvldim, nAdv, fill):
    """the oracle on poisoned inputs == the oracle on the same inputs with fill = 0.0, bit for bit, and is finite"""
    kw = dict(seed=5 * nV + nAdv, nvldim=nvldim, signed_zeros=True)
    poisoned = N.clip_counts(N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, fill=fill, **kw))
    clean = N.clip_counts(N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, fill=0.0, **kw))
    for key in N.INT_KEYS + ("advCoefs", "advCoefs3rd"):
        assert np.array_equal(poisoned[key], clean[key]), key
    differ = poisoned["tracerCur"].view(np.uint64) != clean["tracerCur"].view(np.uint64)
    assert differ.any() and np.all(np.isnan(poisoned["tracerCur"][differ]) if np.isnan(fill)
                                   else poisoned["tracerCur"][differ] == fill)
    a, b = N.high_order_flux(poisoned), N.high_order_flux(clean)
    assert np.all(np.isfinite(a))
    assert_bitwise(a, b, "poisoned vs zero-filled")
    assert nV == 1 or np.any(a != 0.0)            # (nV = 1: the one level has normalThicknessFlux = -0.0)


def test_compact_reproduces_the_oracle_on_sliced_edges(N):
    inp = N.make_inputs_edges(N_EDGES, N_CELLS, 100, 12, seed=9, nvldim=104, fill=float("nan"))
    full = N.high_order_flux(N.clip_counts(inp))
    edges = np.array([66, 0, 1, 14, 15, 40, 13, 13, 30])
    small = N.compact(inp, edges)
    assert small["tracerCur"].shape[1] < N_CELLS and small["advCellsForEdge"].max() <= small["tracerCur"].shape[1]
    assert_bitwise(N.high_order_flux(small), np.asfortranarray(full[:, edges]), "compact")
    bad = dict(inp)
    bad["advCellsForEdge"] = inp["advCellsForEdge"].copy(order="F")
    bad["advCellsForEdge"][0, :] = N_CELLS + 1
    dropped = N.drop_out_of_range_slots(bad)
    assert np.all(dropped["nAdvCellsForEdge"] == np.maximum(N.clip_counts(inp)["nAdvCellsForEdge"] - 1, 0))
    shifted = N.clip_counts(inp)
    for key in ("advCellsForEdge", "advCoefs", "advCoefs3rd"):       # the same problem without slot 1, written by hand
        shifted[key] = np.asfortranarray(np.roll(inp[key], -1, axis=0))
    shifted["nAdvCellsForEdge"] = dropped["nAdvCellsForEdge"]
    assert_bitwise(N.high_order_flux(dropped), N.high_order_flux(shifted), "drop_out_of_range_slots")


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available()
    import codesign_kernels_amd.nlk as nlk_hip
    yield nlk_hip
    nlk_hip.set_variant(nlk_hip.VARIANT_EXACT)
    nlk_hip.set_kernel(-1)


def upload(inp, K, shift=()):
    """device tensors (axes reversed); a key in `shift` is placed one element into a larger allocation (a double
    array then sits at 8 modulo 16, an integer array at 4 modulo 8)"""
    import torch
    d = {}
    for k in K.INT_KEYS + K.REAL_KEYS:
        a = np.ascontiguousarray(np.asarray(inp[k], dtype=np.int32 if k in K.INT_KEYS else np.float64).T)
        t = torch.from_numpy(a).to("cuda:0")
        if k in shift:
            buf = torch.empty(t.numel() + 3, dtype=t.dtype, device="cuda:0")
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % (2 * t.element_size()) == t.element_size() and v.is_contiguous()
            t = v
        d[k] = t
    return d


def new_out(nEdges, nvldim, shifted=False):
    import torch
    if not shifted:
        return torch.full((nEdges, nvldim), PREFILL, dtype=torch.float64, device="cuda:0")
    buf = torch.full((nEdges * nvldim + 3,), PREFILL, dtype=torch.float64, device="cuda:0")
    v = buf[1:1 + nEdges * nvldim].view(nEdges, nvldim)
    assert v.data_ptr() % 16 == 8
    return v


def run(K, d, inp, variant, mode, out=None):
    import torch
    nvldim, nEdges = inp["normalThicknessFlux"].shape
    out = new_out(nEdges, nvldim) if out is None else out
    K.set_variant(variant)
    K.set_kernel(mode)
    K.high_order_flux(d, inp["nVertLevels"], inp["coef3rdOrder"], out)
    torch.cuda.synchronize()
    return np.asfortranarray(out.cpu().numpy().T)


def check(N, out, ref, S, n, nV, variant, what, regime):
    """one result against the oracle: the bars of the module docstring"""
    assert_bitwise(out[nV:], np.full_like(out[nV:], PREFILL), f"{what}: padding rows")
    assert np.all(np.isfinite(out[:nV])), f"{what}: {np.count_nonzero(~np.isfinite(out[:nV]))} non-finite values in written levels"
    if variant == 0:
        assert_bitwise(out[:nV], ref[:nV], what)
        return
    L = np.longdouble
    bound = 2 * np.array([N.gamma(int(m) + 4) for m in n], dtype=L)[None, :] * S
    err = np.abs(out[:nV].astype(L) - ref[:nV].astype(L))
    zero = S == 0
    assert_bitwise(out[:nV][zero], ref[:nV][zero], f"{what}: levels with S = 0")
    ratio = float(np.max(np.where(zero, L(0), err / np.where(zero, L(1), bound)))) if err.size else 0.0
    if ratio > FAST_WORST.get(regime, (0.0, ""))[0]:
        FAST_WORST[regime] = (ratio, what)
    assert np.all(err <= bound), f"{what}: worst |fast - ref| / (2 gamma(n+4) S) = {ratio:.3f}"


def check_all(K, N, inp, what, regime, ref=None, d=None, shifted_out=False):
    """every kernel mode and both variants of one problem; returns the EXACT outputs per mode"""
    nV = inp["nVertLevels"]
    nvldim, nEdges = inp["normalThicknessFlux"].shape
    ref = N.high_order_flux(N.clip_counts(inp)) if ref is None else ref
    S, n = N.abs_sum(inp)
    d = upload(inp, K) if d is None else d
    outs = {}
    for variant in (0, 1):
        for mode in MODES:
            out = run(K, d, inp, variant, mode, new_out(nEdges, nvldim, shifted_out))
            check(N, out, ref, S, n, nV, variant, f"{what} variant={variant} mode={mode}", regime)
            outs[variant, mode] = out
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [-1e34, 1e300, float("nan")], ids=["mpas-fill", "1e300", "nan"])
@pytest.mark.parametrize("nV", NV_SHAPES)
def test_b1_poison_ranges_and_counts(K, N, nV, fill):
    """Fill values in every masked element, every class of level range and of count (test_generator_produces_
    every_class), every leading dimension of nvldims() and nAdv in NADVS (above 64 the vector-bookkeeping form
    cannot run and launch() falls back; for an odd nvldim it must leave the 16-byte forms -- which form ran is
    not observable through the C-ABI, only its result is compared: a missing fall-back for nAdv > 64 corrupts the
    result and is caught, one for an odd nvldim would most likely pass, since the hardware accepts 16-byte
    accesses at 8 modulo 16).  The reference SKIPS a masked level, so no NaN, no 1e300 and no -1e34
    may reach a written level: with fill = NaN a single unmasked read makes the level NaN."""
    for nvldim in nvldims(nV):
        for nAdv in NADVS:
            inp = N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, seed=nV + nAdv, nvldim=nvldim, fill=fill)
            check_all(K, N, inp, f"nV={nV} nvldim={nvldim} nAdv={nAdv} fill={fill}", "poison")


@pytest.mark.gpu
@pytest.mark.parametrize("nV,nvldim,nAdv", [(100, 100, 10), (65, 72, 20), (128, 131, 12), (7, 8, 65)])
def test_b2_cells_out_of_range(K, N, nV, nvldim, nAdv):
    """Cell indices 0, -1, -nCells, nCells+1, 2^31-1 in random slots, slot 1 and the last slot of a full batch of ten
    (or the last slot of the row) included; the table is poisoned.  The header's contract -- such a cell contributes
    nothing -- is the oracle on the problem with those slots deleted and the rows compacted."""
    inp = N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, seed=31 + nV, nvldim=nvldim, fill=-1e34)
    rng = np.random.default_rng(nV)
    bad_values = np.array([0, -1, -N_CELLS, N_CELLS + 1, 2 ** 31 - 1], dtype=np.int32)
    cells = inp["advCellsForEdge"].copy(order="F")
    hit = rng.random(cells.shape) < 0.15
    hit[0, ::3] = True
    hit[min(9, nAdv - 1), 1::3] = True
    hit[nAdv - 1, 2::3] = True
    hit[nAdv - 1, 12:14] = True                       # (edges 12, 13 have the counts nAdv and nAdv + 3: full rows)
    hit[min(9, nAdv - 1), 12:14] = True
    cells[hit] = bad_values[rng.integers(0, 5, int(hit.sum()))]
    inp["advCellsForEdge"] = cells
    live = np.arange(nAdv)[:, None] < N.clip_counts(inp)["nAdvCellsForEdge"][None, :]
    bad_live = live & ((cells < 1) | (cells > N_CELLS))
    assert bad_live[0].any() and bad_live[nAdv - 1].any() and bad_live[min(9, nAdv - 1)].any()   # what the docstring promises
    edges, c = N.referenced(inp)
    assert all(np.any(c + 1 == v) for v in bad_values) and np.any((c >= 0) & (c < N_CELLS))
    ref = N.high_order_flux(N.drop_out_of_range_slots(inp))
    assert np.all(np.isfinite(ref))
    check_all(K, N, inp, f"out-of-range cells nV={nV} nAdv={nAdv}", "bad-cells", ref=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2.0 ** -30, 2.0 ** -10, 1.0, 2.0 ** 12], ids=["2^-30", "2^-10", "1", "2^12"])
def test_b3_scales_cancellation_and_signed_zeros(K, N, scale):
    """All real inputs times a power of two; advCoefs of mixed sign (the sums cancel); normalThicknessFlux holds
    -0.0 and +0.0 (sign(1, -0.0) = -1, nested.F90:128) and subnormals, which are not scaled.  The S-bound is
    homogeneous in the inputs, so the same assertion serves every scale."""
    for nV, nvldim, nAdv in [(100, 100, 10), (63, 64, 12), (129, 134, 20), (2, 2, 65)]:
        inp = N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, seed=77 + nV, nvldim=nvldim, fill=-1e34, scale=scale,
                                  signed_zeros=True)
        ntf = inp["normalThicknessFlux"][:nV]
        assert np.any(np.signbit(ntf) & (ntf == 0)) and np.any(~np.signbit(ntf) & (ntf == 0))
        assert np.any((ntf != 0) & (np.abs(ntf) < np.finfo(np.float64).tiny))
        assert np.any(inp["advCoefs"] < 0) and np.any(inp["advCoefs"] > 0)
        check_all(K, N, inp, f"scale={scale} nV={nV} nAdv={nAdv}", f"scale {scale:g}")


SENTINEL = 0x7FF8DEADBEEF0001                 # a NaN payload pattern, compared as 64-bit integers


@pytest.mark.gpu
@pytest.mark.parametrize("nV,nvldim,nAdv", [(100, 100, 10), (64, 66, 12), (3, 4, 65)])
def test_b4_base_placement_guard_bands_and_inputs_untouched(K, N, nV, nvldim, nAdv):
    """Each of tracerCur, normalThicknessFlux, advMaskHighOrder, highOrderFlx in turn at 8 modulo 16 (launch() is
    meant to leave the 16-byte forms; the test sees results only, not the form taken, and the hardware accepts 16-byte
    accesses at 8 modulo 16, so what is pinned here is that such bases give the same bits, not the choice of kernel),
    then all four; the integer tables at 4 modulo 8 and the coefficient tables at 8 modulo
    16 (they are read with 4- and 8-byte accesses in every form): bit-identical to the aligned run for every mode.
    highOrderFlx inside a buffer with 4 KiB of NaN-payload sentinel on both sides: both bands unchanged.  Every input
    array bit-identical to its copy after all calls."""
    import torch
    inp = N.make_inputs_edges(N_EDGES, N_CELLS, nV, nAdv, seed=3 + nV, nvldim=nvldim, fill=float("nan"))
    aligned = check_all(K, N, inp, "aligned", "placement")
    real4 = ("tracerCur", "normalThicknessFlux", "advMaskHighOrder")
    placements = [(k,) for k in real4] + [("highOrderFlx",), real4 + ("highOrderFlx",),
                                          K.INT_KEYS + ("advCoefs", "advCoefs3rd")]
    for shift in placements:
        d = upload(inp, K, shift=shift)
        outs = check_all(K, N, inp, f"shifted {shift}", "placement", d=d, shifted_out="highOrderFlx" in shift)
        for key, out in outs.items():
            assert_bitwise(out, aligned[key], f"shifted {shift} vs aligned, (variant, mode) = {key}")
    # guard bands and inputs
    d = upload(inp, K)
    copies = {k: t.clone() for k, t in d.items()}
    band = 512                                                        # doubles: 4 KiB
    n = N_EDGES * nvldim
    buf = torch.full((n + 2 * band,), SENTINEL, dtype=torch.int64, device="cuda:0").view(torch.float64)
    out = buf[band:band + n].view(N_EDGES, nvldim)
    assert out.data_ptr() % 16 == 0
    for variant in (0, 1):
        for mode in MODES:
            out.fill_(PREFILL)
            got = run(K, d, inp, variant, mode, out)
            assert_bitwise(got, aligned[variant, mode], f"guarded buffer variant={variant} mode={mode}")
            raw = buf.view(torch.int64)
            assert bool((raw[:band] == SENTINEL).all()) and bool((raw[band + n:] == SENTINEL).all()), (variant, mode)
    for k, t in d.items():
        as_int = (lambda x: x.view(torch.int64)) if t.dtype == torch.float64 else (lambda x: x)
        assert torch.equal(as_int(t), as_int(copies[k])), f"{k} was modified"


# ---- large tables: generated and poisoned on the device, compared through compact() on chosen edges
def need_memory(gib):
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < gib * 2 ** 30:
        pytest.skip(f"memory shortfall: this case needs {gib} GiB of device memory, torch.cuda.mem_get_info reports "
                    f"{free / 2 ** 30:.1f} GiB free")


def device_problem(nEdges, nCells, nV, nvldim, nAdv, seed, fill=-1e34):
    """device tensors of a random problem; tracerCur poisoned by a broadcast level mask"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    dev = "cuda:0"
    maxl = torch.randint(1, nV + 1, (nCells,), device=dev, generator=g, dtype=torch.int32)
    minl = torch.where(torch.rand(nCells, device=dev, generator=g) < 0.5, torch.ones_like(maxl),
                       torch.minimum(torch.randint(1, nV + 1, (nCells,), device=dev, generator=g, dtype=torch.int32), maxl))
    k = torch.arange(1, nvldim + 1, device=dev, dtype=torch.int32)[None, :]
    tr = torch.rand((nCells, nvldim), dtype=torch.float64, device=dev, generator=g)
    tr.mul_(15.0)
    step = 1 << 18                                                   # (in blocks: the mask of the whole table would be another 0.5 GB)
    for c0 in range(0, nCells, step):
        sl = slice(c0, min(c0 + step, nCells))
        tr[sl].masked_fill_(~((k >= minl[sl, None]) & (k <= maxl[sl, None]) & (k <= nV)), fill)
    ntf = torch.rand((nEdges, nvldim), dtype=torch.float64, device=dev, generator=g)
    ntf.sub_(0.5).mul_(-15.0)
    msk = torch.rand((nEdges, nvldim), dtype=torch.float64, device=dev, generator=g)
    msk.lt_(0.9)                                                      # in place: 1.0 / 0.0
    ntf[:, nV:] = fill
    msk[:, nV:] = fill
    return {"nAdvCellsForEdge": torch.randint(1, nAdv + 1, (nEdges,), device=dev, generator=g, dtype=torch.int32),
            "advCellsForEdge": torch.randint(1, nCells + 1, (nEdges, nAdv), device=dev, generator=g, dtype=torch.int32),
            "minLevelCell": minl, "maxLevelCell": maxl, "tracerCur": tr, "normalThicknessFlux": ntf,
            "advMaskHighOrder": msk,
            "advCoefs": (torch.rand((nEdges, nAdv), dtype=torch.float64, device=dev, generator=g) - 0.5) * 20.0,
            "advCoefs3rd": (torch.rand((nEdges, nAdv), dtype=torch.float64, device=dev, generator=g) - 0.5) * 21.0}


def check_device_problem(K, N, d, nV, edges, what, regime):
    """all modes and variants; `edges` (every one of them, every level) against the oracle on compact()"""
    import torch
    nEdges, nvldim = d["normalThicknessFlux"].shape
    meta = {"coef3rdOrder": N.coef3rd(), "nVertLevels": nV}
    idx = torch.as_tensor(np.asarray(edges), device="cuda:0", dtype=torch.int64)

    def fetch(key, i):
        t = d[key].index_select(0, torch.as_tensor(np.asarray(i), device="cuda:0", dtype=torch.int64))
        return np.asfortranarray(t.cpu().numpy().T)

    small = N.compact(meta, edges, fetch=fetch)
    ref = N.high_order_flux(small)
    assert np.all(np.isfinite(ref))
    S, n = N.abs_sum(small)
    out = torch.empty((nEdges, nvldim), dtype=torch.float64, device="cuda:0")
    for variant in (0, 1):
        for mode in MODES:
            out.fill_(PREFILL)
            K.set_variant(variant)
            K.set_kernel(mode)
            K.high_order_flux(d, nV, meta["coef3rdOrder"], out)
            torch.cuda.synchronize()
            got = np.asfortranarray(out.index_select(0, idx).cpu().numpy().T)
            check(N, got, ref, S, n, nV, variant, f"{what} variant={variant} mode={mode}", regime)


def plant_cells(d, nCells, nvldim, byte_marks):
    """the first edges reference, in slot 1 with a count of at least 1: cell 1, the last three cells, and every cell
    whose column straddles or neighbours byte offsets mark - 1024 .. mark + 1024 of tracerCur"""
    import torch
    col = nvldim * 8
    want = [1, nCells - 2, nCells - 1, nCells]
    for mark in byte_marks:
        want += [c + 1 for c in range((mark - 1024) // col - 1, (mark + 1024) // col + 2) if 0 <= c < nCells]
    want = sorted(set(want))
    t = torch.as_tensor(want, dtype=torch.int32, device="cuda:0")
    d["advCellsForEdge"][:len(want), 0] = t
    d["advCellsForEdge"][len(want):2 * len(want), -1] = t             # ... and in the last slot of a full row
    d["nAdvCellsForEdge"][len(want):2 * len(want)] = d["advCellsForEdge"].shape[1]
    return want


@pytest.mark.gpu
def test_b5_tracer_table_between_2_and_4_gib(K, N):
    """nvldim = 128, nCells = 3.5 M: a tracerCur of 3.58 GB, so the 32-bit column offsets of the two-level forms are
    taken and cross 2^31.  4096 edges reference cell 1, the cells around byte offset 2^31, the last three cells and
    random cells; all of them are compared.  Needs 8 GiB of device memory."""
    need_memory(8)
    nCells, nvldim, nV, nAdv, nEdges = 3_500_000, 128, 125, 10, 4096
    assert 2 ** 31 < nCells * nvldim * 8 < 4294967000
    d = device_problem(nEdges, nCells, nV, nvldim, nAdv, seed=21)
    plant_cells(d, nCells, nvldim, [2 ** 31])
    check_device_problem(K, N, d, nV, np.arange(nEdges), "tracerCur 3.58 GB", "large")


@pytest.mark.gpu
def test_b5_tracer_table_above_4_gib(K, N):
    """nCells = 4.3 M at nvldim = 128: 4.40 GB, beyond 32-bit column offsets -- every mode must fall back to the form
    with 64-bit column addresses (checked through the results: without the fall-back the offsets of the cells beyond
    2^32 bytes wrap and their columns come from the wrong cells).  Same edge recipe, plus the cells around byte offset 2^32.  Needs 10 GiB."""
    need_memory(10)
    nCells, nvldim, nV, nAdv, nEdges = 4_300_000, 128, 125, 10, 4096
    assert nCells * nvldim * 8 > 2 ** 32
    d = device_problem(nEdges, nCells, nV, nvldim, nAdv, seed=22)
    plant_cells(d, nCells, nvldim, [2 ** 31, 2 ** 32])
    check_device_problem(K, N, d, nV, np.arange(nEdges), "tracerCur 4.40 GB", "large")


@pytest.mark.gpu
def test_b5_edge_arrays_above_4_gib(K, N):
    """nvldim = 256, nEdges = 2^21 + 4096: each of normalThicknessFlux, advMaskHighOrder, highOrderFlx is 4.30 GB.
    Whole blocks of 256 edges are compared at the start, around the 2^31-byte and the 2^32-byte crossing of a row
    array, and at the end: 1024 edges, every level.  Needs 16 GiB."""
    need_memory(16)
    nEdges, nvldim, nV, nAdv, nCells = 2 ** 21 + 4096, 256, 250, 4, 1000
    assert nEdges * nvldim * 8 > 2 ** 32
    d = device_problem(nEdges, nCells, nV, nvldim, nAdv, seed=23)
    row = nvldim * 8
    blocks = [0, 2 ** 31 // row - 128, 2 ** 32 // row - 128, nEdges - 256]
    edges = np.concatenate([np.arange(b, b + 256) for b in blocks])
    assert len(set(edges)) == 1024 and edges.max() == nEdges - 1
    check_device_problem(K, N, d, nV, edges, "edge arrays 4.30 GB", "large")


@pytest.mark.gpu
def test_report_fast_ratios():
    """(runs last in this module) the worst FAST ratio |fast - ref| / (2 gamma(n+4) S) per regime, for the record"""
    for regime, (ratio, what) in sorted(FAST_WORST.items()):
        print(f"NLK FAST {regime:12s} worst |fast - ref| / (2 gamma(n+4) S) = {ratio:.4f}   ({what})")
    assert FAST_WORST and all(r <= 1.0 for r, _ in FAST_WORST.values())
