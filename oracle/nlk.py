"""oracle/nlk.py -- TEST INFRASTRUCTURE: Python face of the CPU oracle of the third mini-app
(nested_loops/nested.F90: MPAS-Ocean high-order tracer flux gather).  Wraps
oracle/libnlk_oracle.so (nlk_oracle.c) and oracle/_ref/nlk_ref (the reference program itself,
built by build_ref.py --nlk).  Only tests/, smoke() and bench.py's cpu_baseline leg import it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from oracle.rounding import GAMMA_U, gamma  # noqa: F401  (the FAST bound 2 * gamma(n + 4) * S, abs_sum below)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnlk_oracle.so")
REF_EXE = os.path.join(HERE, "_ref", "nlk_ref")
INT_KEYS = ("nAdvCellsForEdge", "advCellsForEdge", "minLevelCell", "maxLevelCell")
REAL_KEYS = ("tracerCur", "normalThicknessFlux", "advMaskHighOrder", "advCoefs", "advCoefs3rd")
_lib = None


def build_lib(force=False):
    src = os.path.join(HERE, "nlk_oracle.c")
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= os.path.getmtime(src):
        return LIB_PATH
    subprocess.run(["gcc", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB_PATH, src, "-lm"], check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build_lib()
        L = ctypes.CDLL(LIB_PATH)
        ip, dp, ci = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_int
        L.nlk_oracle_high_order_flux.restype = ci
        L.nlk_oracle_high_order_flux.argtypes = [ci] * 5 + [ip] * 4 + [dp] * 5 + [ctypes.c_double, dp]
        L.nlk_oracle_coef3rd.restype = ctypes.c_double
        _lib = L
    return _lib


def coef3rd():
    """coef3rdOrder as the reference holds it (nested_vars.F90:35: the fp32 value of 2.14)."""
    return lib().nlk_oracle_coef3rd()


def make_inputs(nEdges, nCells, nVertLevels, nAdv, seed, nvldim=None, ragged=True):
    """Inputs in the spirit of the reference's initialisation (nested.F90:58-108): random
    connectivity, topography with about half the cells at full depth; `ragged` also varies
    nAdvCellsForEdge and minLevelCell (the reference keeps them at nAdv and 1)."""
    rng = np.random.default_rng(seed)
    nvldim = nVertLevels if nvldim is None else nvldim
    maxl = np.minimum(np.maximum(3, np.rint(rng.random(nCells) * nVertLevels * 2.0)), nVertLevels).astype(np.int32)
    maxl = np.minimum(maxl, nVertLevels)
    minl = np.ones(nCells, np.int32)
    if ragged:
        minl = np.minimum(rng.integers(1, 4, nCells), maxl).astype(np.int32)
    tr = np.zeros((nvldim, nCells), order="F")
    for c in range(nCells):
        tr[minl[c] - 1:maxl[c], c] = 15.0 * rng.random(maxl[c] - minl[c] + 1)
    nadv = np.full(nEdges, nAdv, np.int32)
    if ragged:
        nadv = rng.integers(1, nAdv + 1, nEdges).astype(np.int32)
    inp = {"nAdvCellsForEdge": nadv,
           "advCellsForEdge": np.asfortranarray(rng.integers(1, nCells + 1, (nAdv, nEdges)).astype(np.int32)),
           "minLevelCell": minl, "maxLevelCell": maxl, "tracerCur": tr,
           "normalThicknessFlux": np.asfortranarray(15.0 * (0.5 - rng.random((nvldim, nEdges)))),
           "advMaskHighOrder": np.asfortranarray((rng.random((nvldim, nEdges)) < 0.9).astype(np.float64) if ragged
                                                 else np.ones((nvldim, nEdges))),
           "advCoefs": np.asfortranarray(20.0 * rng.random((nAdv, nEdges))),
           "advCoefs3rd": np.asfortranarray(21.0 * rng.random((nAdv, nEdges))),
           "coef3rdOrder": coef3rd(), "nVertLevels": nVertLevels}
    return inp


def high_order_flux(inp):
    """C restatement of the reference loop (nested.F90:123-157) -> highOrderFlx(nvldim,nEdges);
    rows nVertLevels+1..nvldim stay 0."""
    nvldim, nEdges = inp["normalThicknessFlux"].shape
    nCells = inp["tracerCur"].shape[1]
    nAdv = inp["advCellsForEdge"].shape[0]
    out = np.zeros((nvldim, nEdges), order="F")
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    ia = [np.asfortranarray(inp[k], dtype=np.int32) for k in INT_KEYS]
    ra = [np.asfortranarray(inp[k], dtype=np.float64) for k in REAL_KEYS]
    rc = lib().nlk_oracle_high_order_flux(nEdges, nCells, inp["nVertLevels"], nvldim, nAdv,
                                          *[a.ctypes.data_as(ip) for a in ia], *[a.ctypes.data_as(dp) for a in ra],
                                          float(inp["coef3rdOrder"]), out.ctypes.data_as(dp))
    if rc:
        raise RuntimeError(f"nlk_oracle_high_order_flux failed rc={rc}")
    return out


def run_reference(nEdges, nCells, nVertLevels, nAdv, seed):
    """Run the reference program on a seeded random stream; returns (inputs as the program built
    them, its refFlx)."""
    if not os.path.exists(REF_EXE):
        raise FileNotFoundError("no oracle/_ref/nlk_ref")
    nrand = nCells * (1 + nVertLevels) + nEdges * (3 * nAdv + nVertLevels) + 16
    with tempfile.TemporaryDirectory(prefix="nlk_refrun_") as tmp:
        with open(os.path.join(tmp, "nested.nml"), "w") as fh:
            fh.write(f"&nested_nml\n nIters = 1\n nEdges = {nEdges}\n nCells = {nCells}\n"
                     f" nVertLevels = {nVertLevels}\n nAdv = {nAdv}\n/\n")
        np.random.default_rng(seed).random(nrand).tofile(os.path.join(tmp, "nlk_rand.bin"))
        subprocess.run([REF_EXE], cwd=tmp, check=True, capture_output=True, text=True)
        raw = open(os.path.join(tmp, "nlk_out.bin"), "rb").read()
    off = 0

    def take(dtype, shape):
        nonlocal off
        n = int(np.prod(shape))
        a = np.frombuffer(raw, dtype=dtype, count=n, offset=off).reshape(shape, order="F").copy(order="F")
        off += n * np.dtype(dtype).itemsize
        return a

    nE, nC, nV, nvldim, nA = (int(x) for x in take(np.int32, (5,)))
    inp = {"nAdvCellsForEdge": take(np.int32, (nE,)), "advCellsForEdge": take(np.int32, (nA, nE)),
           "minLevelCell": take(np.int32, (nC,)), "maxLevelCell": take(np.int32, (nC,)),
           "tracerCur": take(np.float64, (nvldim, nC)), "normalThicknessFlux": take(np.float64, (nvldim, nE)),
           "advMaskHighOrder": take(np.float64, (nvldim, nE)), "advCoefs": take(np.float64, (nA, nE)),
           "advCoefs3rd": take(np.float64, (nA, nE))}
    inp["coef3rdOrder"] = float(take(np.float64, (1,))[0])
    inp["nVertLevels"] = nV
    ref = take(np.float64, (nvldim, nE))
    return inp, ref


# ------------------------------------------------------------------ adversarial inputs
FILLS = (-1e34, 1e300, float("nan"))                     # the MPAS fill value, a value whose products overflow, NaN
COUNT_CLASSES = (0, -2, 1, 4, 5, 6, 9, 10, 11, 19, 20, 21)   # + nAdv, nAdv + 3 (make_inputs_edges)
LEVEL_BOUNDARIES = (63, 64, 65, 127, 128, 129)           # trip boundaries of the kernels' 64 / 128-level trips


def range_classes(nVertLevels, nvldim):
    """(minLevelCell, maxLevelCell) pairs that make_inputs_edges gives its first cells: every class of level range
    that the reference's test `minLevelCell <= k <= maxLevelCell` (nested.F90:139) can meet."""
    nV, mid = nVertLevels, max(1, nVertLevels // 2)
    rc = [(1, 0), (1, -3), (1, nvldim + 5), (2, nvldim + 5), (mid + 1, mid), (nV + 2, nV), (0, nV), (-2, nV),
          (1, 1), (nV, nV), (mid, mid), (1, nV)]
    if nvldim > nV:
        rc += [(1, nV + 1), (1, nvldim)]                 # maxLevelCell in (nVertLevels, nvldim]
    if nV >= 2:
        odd, even = (nV - 1) | 1, nV & ~1                # the largest odd / even level <= nV
        rc += [(1, min(odd, nV)), (1, even), (2, nV)]
    if nV >= 3:
        rc += [(3, nV - 1 if nV - 1 >= 3 else nV)]
    for b in LEVEL_BOUNDARIES:
        if b <= nV:
            rc += [(1, b), (b, nV), (b, b)]
    return rc


def make_inputs_edges(nEdges, nCells, nVertLevels, nAdv, seed, nvldim=None, fill=-1e34, scale=1.0, signed_zeros=False):
    """Adversarial inputs for the flux gather.  `fill` sits in every tracerCur element outside its cell's
    [minLevelCell, maxLevelCell] (rows nVertLevels+1..nvldim and whole columns of cells with an empty range
    included) and in the padding rows of normalThicknessFlux and advMaskHighOrder: everywhere the reference
    (nested.F90:123-157) never reads.  The first cells take range_classes(), the first edges the count classes
    COUNT_CLASSES + (nAdv, nAdv+3); every class cell sits in slot 1 of an edge with a count >= 1, so it is
    referenced.  advCoefs / advCoefs3rd have mixed sign (the sums cancel); all real inputs are multiplied by `scale`
    (a power of two); `signed_zeros` puts -0.0, +0.0 and unscaled subnormals into normalThicknessFlux.  Every random
    draw is independent of `fill`, so two calls that differ only in `fill` differ only in the poisoned elements.
    Counts are NOT clipped (clip_counts) -- the oracle does not clip."""
    rng = np.random.default_rng(seed)
    nV = nVertLevels
    nvldim = nV if nvldim is None else nvldim
    rc = range_classes(nV, nvldim)
    counts = list(COUNT_CLASSES) + [nAdv, nAdv + 3]
    if nCells < len(rc) + 4 or nEdges < len(counts) + len(rc) + 4:
        raise ValueError(f"need nCells >= {len(rc) + 4} and nEdges >= {len(counts) + len(rc) + 4}")
    maxl = rng.integers(1, nV + 1, nCells).astype(np.int32)
    minl = np.where(rng.random(nCells) < 0.5, 1, rng.integers(1, nV + 1, nCells)).astype(np.int32)
    minl = np.minimum(minl, maxl)
    for c, (lo, hi) in enumerate(rc):
        minl[c], maxl[c] = lo, hi
    k = np.arange(1, nvldim + 1)[:, None]
    inside = (k >= minl[None, :]) & (k <= maxl[None, :]) & (k <= nV)
    tr = np.asfortranarray(np.where(inside, scale * 15.0 * rng.random((nvldim, nCells)), fill))
    nadv = rng.integers(1, nAdv + 1, nEdges).astype(np.int32)
    nadv[:len(counts)] = counts
    cells = rng.integers(1, nCells + 1, (nAdv, nEdges)).astype(np.int32)
    for c in range(len(rc)):
        cells[0, len(counts) + c] = c + 1
    pad = k > nV
    ntf = scale * 15.0 * (0.5 - rng.random((nvldim, nEdges)))
    if signed_zeros:
        z = rng.random((nvldim, nEdges))
        ntf = np.where(z < 0.05, -0.0, np.where(z < 0.10, 0.0, ntf))
        ntf = np.where((z >= 0.10) & (z < 0.13), np.float64(2.0 ** -1040) * (rng.random((nvldim, nEdges)) - 0.5), ntf)
        ntf[0, :] = -0.0                                  # sign(1.0, -0.0) = -1 (nested.F90:128)
    msk = np.where(rng.random((nvldim, nEdges)) < 0.9, scale, 0.0)
    return {"nAdvCellsForEdge": nadv, "advCellsForEdge": np.asfortranarray(cells),
            "minLevelCell": minl, "maxLevelCell": maxl, "tracerCur": tr,
            "normalThicknessFlux": np.asfortranarray(np.where(pad, fill, ntf)),
            "advMaskHighOrder": np.asfortranarray(np.where(pad, fill, msk)),
            "advCoefs": np.asfortranarray(scale * 20.0 * (rng.random((nAdv, nEdges)) - 0.5)),
            "advCoefs3rd": np.asfortranarray(scale * 21.0 * (rng.random((nAdv, nEdges)) - 0.5)),
            "coef3rdOrder": coef3rd(), "nVertLevels": nV}


def clip_counts(inp):
    """A copy of `inp` with nAdvCellsForEdge = min(max(n, 0), nAdv): what the library promises for counts
    outside 0..nAdv (the oracle does not clip and would read past the row)."""
    out = dict(inp)
    out["nAdvCellsForEdge"] = np.clip(inp["nAdvCellsForEdge"], 0, inp["advCellsForEdge"].shape[0]).astype(np.int32)
    return out


def referenced(inp):
    """(edge indices, 0-based cell indices) of every slot below its edge's clipped count"""
    nAdv, nEdges = inp["advCellsForEdge"].shape
    n = clip_counts(inp)["nAdvCellsForEdge"]
    live = np.arange(nAdv)[:, None] < n[None, :]
    return np.nonzero(live)[1], inp["advCellsForEdge"][live] - 1


def edge_classes(inp):
    """Which of the classes of the issue occur among the cells and edges that the gather really visits:
    dict name -> bool (the generator self-check asserts them all)."""
    nV, nvldim = inp["nVertLevels"], inp["tracerCur"].shape[0]
    nAdv = inp["advCellsForEdge"].shape[0]
    _, c = referenced(inp)
    lo, hi = inp["minLevelCell"][c], inp["maxLevelCell"][c]
    cl = {"max=0": np.any(hi == 0), "max<0": np.any(hi < 0), "max>nvldim": np.any(hi > nvldim),
          "min>max": np.any((lo > hi) & (hi >= 1)), "min>nV": np.any(lo > nV),
          "min<=0": np.any(lo <= 0), "min=max": np.any((lo == hi) & (lo >= 1) & (lo <= nV))}
    if nvldim > nV:
        cl["nV<max<=nvldim"] = np.any((hi > nV) & (hi <= nvldim))
    if nV >= 2:
        cl["max odd"] = np.any((hi % 2 == 1) & (hi >= 1) & (hi <= nV))
        cl["max even"] = np.any((hi % 2 == 0) & (hi >= 1) & (hi <= nV))
        cl["min>1"] = np.any((lo > 1) & (lo <= hi))
    for b in LEVEL_BOUNDARIES:
        if b <= nV:
            cl[f"max={b}"] = np.any(hi == b)
            cl[f"min={b}"] = np.any((lo == b) & (lo <= hi))
    for n in list(COUNT_CLASSES) + [nAdv, nAdv + 3]:
        cl[f"count={n}"] = np.any(inp["nAdvCellsForEdge"] == n)
    cl["count<0"] = np.any(inp["nAdvCellsForEdge"] < 0)
    return {k: bool(v) for k, v in cl.items()}


def compact(inp, edges, fetch=None):
    """The problem that holds only `edges` (in that order) and the cells they reference, indices remapped.
    Cells are independent columns, so the oracle's result on it is bit for bit the result of the full problem
    on those edges.  Counts come out clipped; slots at or above the count (never read) point at cell 1.
    `fetch(key, idx)` returns columns `idx` (last Fortran axis) of array `key` as a Fortran-ordered numpy array;
    the default reads them from `inp` (a test with device-resident tables passes its own)."""
    if fetch is None:
        fetch = lambda key, idx: np.asfortranarray(inp[key][..., idx])
    edges = np.asarray(edges, dtype=np.int64)
    cells = np.array(fetch("advCellsForEdge", edges), dtype=np.int64, order="F")
    nAdv = cells.shape[0]
    n = np.clip(np.asarray(fetch("nAdvCellsForEdge", edges)), 0, nAdv).astype(np.int32)
    live = np.arange(nAdv)[:, None] < n[None, :]
    used = np.unique(cells[live]) - 1                     # 0-based cells, ascending
    if used.size == 0:
        used = np.zeros(1, np.int64)
    new = np.ones_like(cells)
    new[live] = np.searchsorted(used, cells[live] - 1) + 1
    out = {"nAdvCellsForEdge": n, "advCellsForEdge": np.asfortranarray(new.astype(np.int32)),
           "coef3rdOrder": inp["coef3rdOrder"], "nVertLevels": inp["nVertLevels"]}
    for key in ("minLevelCell", "maxLevelCell", "tracerCur"):
        out[key] = fetch(key, used)
    for key in ("normalThicknessFlux", "advMaskHighOrder", "advCoefs", "advCoefs3rd"):
        out[key] = fetch(key, edges)
    return out


def drop_out_of_range_slots(inp):
    """A copy of `inp` in which every slot below the (clipped) count whose cell index lies outside 1..nCells is
    DELETED: the later slots of the edge move down, the count shrinks.  The header's contract for such a cell
    ("contributes nothing") is exactly the reference loop on this problem."""
    nAdv, nEdges = inp["advCellsForEdge"].shape
    nCells = inp["tracerCur"].shape[1]
    out = clip_counts(inp)
    n = out["nAdvCellsForEdge"].copy()
    cells = np.ones((nAdv, nEdges), np.int32, order="F")
    c1, c3 = np.zeros((nAdv, nEdges), order="F"), np.zeros((nAdv, nEdges), order="F")
    for e in range(nEdges):
        col = inp["advCellsForEdge"][:n[e], e]
        keep = np.nonzero((col >= 1) & (col <= nCells))[0]
        m = len(keep)
        cells[:m, e], c1[:m, e], c3[:m, e] = col[keep], inp["advCoefs"][keep, e], inp["advCoefs3rd"][keep, e]
        n[e] = m
    out.update(nAdvCellsForEdge=n, advCellsForEdge=cells, advCoefs=c1, advCoefs3rd=c3)
    return out


def abs_sum(inp):
    """S(nVertLevels, nEdges) in np.longdouble: sum over the contributing cells (clipped count, level inside the
    cell's range, cell index in range) of |tracer| * |ntf * mask| * (|advCoefs| + |advCoefs3rd * coef3rdOrder|) --
    the condition-number sum of the gather, for the FAST bound 2 * gamma(n + 4) * S.  Also returns n(nEdges)."""
    L = np.longdouble
    nV = inp["nVertLevels"]
    nAdv, nEdges = inp["advCellsForEdge"].shape
    nCells = inp["tracerCur"].shape[1]
    n = clip_counts(inp)["nAdvCellsForEdge"]
    k = np.arange(1, nV + 1)[:, None]
    w = np.abs(inp["normalThicknessFlux"][:nV].astype(L) * inp["advMaskHighOrder"][:nV].astype(L))
    S = np.zeros((nV, nEdges), L)
    for i in range(nAdv):
        c = inp["advCellsForEdge"][i].astype(np.int64)
        ok = (i < n) & (c >= 1) & (c <= nCells)
        ic = np.where(ok, c - 1, 0)
        on = ok[None, :] & (k >= inp["minLevelCell"][ic][None, :]) & (k <= inp["maxLevelCell"][ic][None, :])
        coef = np.abs(inp["advCoefs"][i].astype(L)) + np.abs(inp["advCoefs3rd"][i].astype(L) * L(inp["coef3rdOrder"]))
        t = np.abs(np.where(on, inp["tracerCur"][:nV][:, ic], 0.0).astype(L))
        S += np.where(on, t * w * coef[None, :], L(0))
    return S, n
