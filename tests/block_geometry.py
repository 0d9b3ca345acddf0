"""What tests/test_block_calls_geometry.py (GPU) and tests/test_block_calls_geometry_cpu.py share: the cases of the six
calls on a block of instances (include/mpdata_hip.h 3g .. 3l) at sizes beyond one thread block, beyond 65535 rows, at
hundreds of tiles and beyond 2^32 bytes; their inputs; the launch geometry restated from csrc/mpdata_wm_walk.h (the tile
grid and the column groups) and csrc/mpdata_diffuse.hip; and `Truth`, the six numpy models applied to blocks of
reference-layout arrays.  The models themselves are those of tests/*_model.py, unchanged.
"""
import numpy as np

import column_path_model as CP
import courant_model as CM
import diffuse_model as DM
import level_add_model as AM
import level_stats_model as LM
import scale_uw_model as SM
from util import bits  # (the tests take it from here)

F64, F32 = np.float64, np.float32
TB = 256            # threads of a block of the reference-layout kernels (x: instances)
YMAX = 65535        # ref_block_grid's cap of gridDim.y (rows)


# ---- inputs: drawn per element, so no two instances, rows or levels are alike.  f: signed, a full mantissa, columns
# scaled by 2**-(column mod 4) (exact; the rounding of a partial sum then depends on the order); u, w in (-1/32, 1/32):
# the outflow Courant number stays below 1/2; rho, adz, rhow in [0.5, 1): 1 / (rho * adz) <= 4 (tests/diffuse_model.py).
def make_inputs(shape, T, dtype, seed):
    """the seven arrays of a problem (ncrms, nx, nz) with T tracers, Fortran order; f and flux ALWAYS carry the tracer axis"""
    ncrms, nx, nz = shape
    nzm = nz - 1
    rng = np.random.default_rng([seed, ncrms, nx, nz, T])
    col = (2.0 ** -(np.arange(nx + 6) % 4))[None, :, None, None]
    sh = (ncrms, nx + 6, nzm, T)
    out = {"f": rng.uniform(-1.0, 1.0, sh) * rng.uniform(0.5, 1.0, sh) * col,
           "u": rng.uniform(-1.0, 1.0, (ncrms, nx + 5, nzm)) / 32, "w": rng.uniform(-1.0, 1.0, (ncrms, nx + 4, nz)) / 32,
           "rho": rng.uniform(0.5, 1.0, (ncrms, nzm)), "rhow": rng.uniform(0.5, 1.0, (ncrms, nz)),
           "adz": rng.uniform(0.5, 1.0, (ncrms, nzm)), "flux": np.zeros((ncrms, nz, T))}
    out = {k: np.asfortranarray(v.astype(dtype)) for k, v in out.items()}
    assert np.all(out["f"] != 0) and np.all(out["w"][:, :, -1] != 0)
    return out


def plan_arrays(inp):
    """the arrays as Plan.upload takes them: one tracer without the tracer axis"""
    T = inp["f"].shape[-1]
    return {k: (np.asfortranarray(v[..., 0]) if k in ("f", "flux") and T == 1 else v) for k, v in inp.items()}


class Truth:
    """The reference-layout arrays a plan (or a set of device arrays) must hold, and the six models on a block [sl0, sl0 + n)
    and a tracer range: the read-only calls return what the call must write, the in-place ones also update the arrays.
    Outputs carry the tracer axis."""

    def __init__(self, inp):
        self.f = np.array(inp["f"], order="F")
        self.u, self.w = np.array(inp["u"], order="F"), np.array(inp["w"], order="F")
        self.rho, self.adz = inp["rho"], inp["adz"]
        self.shape = (self.f.shape[0], self.f.shape[1] - 6, self.f.shape[2] + 1)
        self.T, self.dt = self.f.shape[3], self.f.dtype.type

    def _blk(self, sl0, n, first, ntr):
        n = self.shape[0] - sl0 if n is None else n
        ntr = self.T - first if ntr is None else ntr
        return slice(sl0, sl0 + n), slice(first, first + ntr)

    def stats(self, sl0=0, n=None, first=0, ntr=None):
        b, t = self._blk(sl0, n, first, ntr)
        return dict(zip(("sum", "min", "max"), LM.level_stats(self.f[b, ..., t])))

    def courant(self, sl0=0, n=None):
        b, _ = self._blk(sl0, n, 0, None)
        clev, cinst = CM.courant(self.u[b], self.w[b], self.rho[b], self.adz[b])
        return {"clev": clev, "cinst": cinst}

    def paths(self, sl0=0, n=None, first=0, ntr=None):
        b, t = self._blk(sl0, n, first, ntr)
        return CP.column_path(self.f[b, ..., t], self.rho[b], self.adz[b])

    def add(self, d, sl0=0, n=None, first=0, ntr=None, clip=False):
        b, t = self._blk(sl0, n, first, ntr)
        blk = self.f[b, ..., t]
        self.f[b, ..., t] = AM.level_add(blk, np.asarray(d).reshape(blk.shape[:1] + blk.shape[2:], order="F"), clip)

    def scale(self, su=None, sw=None, sl0=0, n=None):
        b, _ = self._blk(sl0, n, 0, None)
        self.u[b], self.w[b] = SM.scale_uw(self.u[b], self.w[b], su, sw)

    def diffuse(self, c, sl0=0, n=None, first=0, ntr=None):
        b, t = self._blk(sl0, n, first, ntr)
        new, zflux = DM.diffuse(self.f[b, ..., t], self.rho[b], self.adz[b], **c)
        self.f[b, ..., t] = new
        return zflux


def make_d(shape, ntr, dtype, seed, n):
    """level_add_model.make_d with the tracer axis kept: (n, nzm, ntr)"""
    d = AM.make_d(shape, ntr, dtype, seed, n)
    return np.asfortranarray(d.reshape((n, shape[2] - 1, ntr), order="F"))


# ---- launch geometry, restated from the kernels' sources
def slp_of(nz):
    """8-byte elements of the instance axis per tile of a wave-major plan (mpdata_plan.hip: 64 / LPS; one above 64 levels)"""
    return LM._tile(nz, F64) if nz <= 64 else 1


def wm_geometry(shape, dtype, sl0, n, ntr, W=1, nz_w=None):
    """wm_block_grid of mpdata_wm_walk.h for a block of a wave-major plan; W, nz_w: the level windows of a tall plan and
    the levels of one window -> dict(spt, ntiles, t0, t1, ntile, nslice, waves, blocks)"""
    ncrms, nx, nz = shape
    ipe = 2 if np.dtype(dtype) == np.dtype(F32) else 1
    nzi = nz if W == 1 else nz_w
    slp = slp_of(nzi)
    spt = slp * ipe
    elems = (ncrms + ipe - 1) // ipe * W
    chunk = slp * (nzi - 1)
    t0, t1 = sl0 * W // spt, ((sl0 + n) * W - 1) // spt
    nslice = (chunk + 63) // 64
    waves = ntr * (t1 - t0 + 1) * nslice
    return dict(spt=spt, slp=slp, ntiles=(elems + slp - 1) // slp, t0=t0, t1=t1, ntile=t1 - t0 + 1, nslice=nslice, waves=waves,
                blocks=(waves + 3) // 4)


def column_path_geometry(shape, dtype, sl0, n, W=1, nz_w=None):
    """col_groups_batched of mpdata_wm_walk.h as mpdata_column_path.hip calls it (4096 elements of LDS, one coefficient
    row) -> dict(UG, CB, ncb, ngroup)"""
    ncrms, nx, nz = shape
    g = wm_geometry(shape, dtype, sl0, n, 1, W, nz_w)
    slp, ns = g["slp"], ((nz if W == 1 else nz_w) - 1) | 1
    LDS = 4096
    UG = 4 * slp if slp >= 8 else 16
    while UG > slp and UG * ns * 2 > LDS:
        UG //= 2
    cbmax = min(LDS // (UG * ns) - 1, 256 // UG, nx)
    ncb = (nx + cbmax - 1) // cbmax
    first, last = g["t0"] // W * slp, g["t1"] // W * slp + slp - 1
    return dict(UG=UG, CB=(nx + ncb - 1) // ncb, ncb=ncb, ngroup=last // UG - first // UG + 1)


def diffuse_groups(shape, dtype, sl0, n):
    """workgroups per tracer of wm_diffuse_kernel: a group is 4 / nslice whole tiles"""
    g = wm_geometry(shape, dtype, sl0, n, 1)
    tpw = 4 // g["nslice"]
    return (g["ntile"] + tpw - 1) // tpw


# ---- A. the instance axis of the reference-layout kernels: name -> (shape, tracers, dtype, switches, blocks)
BLOCKS_600 = [(0, None), (255, 2), (200, 300), (256, 256), (-1, 1)]          # (-1: the last instance)
REF_KINDS = {
    "f64-ref-n257": ((257, 3, 5), 2, F64, dict(ref=True), [(0, None), (1, 256)]),
    "f32-ref-n257": ((257, 4, 6), 2, F32, dict(ref=True), [(0, None)]),
    "f64-ref-n300": ((300, 4, 8), 2, F64, dict(ref=True), [(0, None), (30, 270)]),
    "f32-ref-n300": ((300, 3, 9), 2, F32, dict(ref=True), [(0, None)]),
    "f64-ref-n600": ((600, 5, 12), 2, F64, dict(ref=True), BLOCKS_600),
    "f32-ref-n600": ((600, 5, 12), 2, F32, dict(ref=True), BLOCKS_600),
    "f32-n601-odd-no-switch": ((601, 3, 7), 2, F32, {}, BLOCKS_600),     # keeps the reference layout
}
ARRAY_A = [(ncrms, dt) for dt in (F64, F32) for ncrms in (257, 300, 600)]
ARRAY_A_SHAPE = {257: (3, 5), 300: (4, 8), 600: (5, 12)}                  # ncrms -> (nx, nz); two tracers

# ---- B. the row loop of the array forms (3 instances): call group -> (shape, tracers); rows per kernel in rows_of
ROW_CASES = {
    # rows = nlev * ntr = 4 * 16385 = 65540: the second trip is rows 65535 .. 65539 -- the last level of tracer 16383
    # and all of tracer 16384
    "f-rows-tracers": ((3, 2, 5), 16385),
    "f-rows-one-tracer": ((3, 1, 65538), 1),      # nzm = 65537: the wrapped rows have vertical neighbours on both sides
    "uw-rows": ((3, 2, 65538), 1),                # nzm = 65537 (u, Courant), nz = 65538 (w)
    "path-rows": ((3, 3, 3), 21846),              # nx * ntr = 65538
    "path-mass-rows": ((3, 1, 4), 65537),         # nx * ntr = ntr = 65537: both passes
}


def rows_of(case):
    """{kernel: rows} of ROW_CASES[case]"""
    (ncrms, nx, nz), T = ROW_CASES[case]
    nzm = nz - 1
    if case.startswith("f-rows"):
        return {"stats": nzm * T, "level_add": nzm * T, "diffuse": nzm * T}
    if case == "uw-rows":
        return {"courant": nzm, "scale_u": nzm, "scale_w": nz}
    return {"path": nx * T, "mass": T} if case == "path-mass-rows" else {"path": nx * T}


# ---- C. wave-major plans at hundreds of workgroups: name -> (shape, tracers, dtype, switches, blocks (sl0, n, first, ntr))
WM_KINDS = {
    # two instances per tile: 301 tiles, the last one half padding
    "f64-n601-nx32-nz28": ((601, 32, 28), 3, F64, {}, [(0, 601, 0, 3), (401, 150, 1, 2), (77, 418, 2, 1), (600, 1, 0, 3)]),
    # four per tile (two pairs): 151 tiles, the last pair half phantom; 401 + 150 = 551: pairs split at both ends
    "f32-n601-nx32-nz28-odd": ((601, 32, 28), 2, F32, dict(odd=True), [(0, 601, 0, 2), (401, 150, 1, 1), (77, 418, 0, 1), (600, 1, 0, 2)]),
    # 16 per tile: 65 tiles (the deepest start there is: tile 50)
    "f32-n1030-nx8-nz6": ((1030, 8, 6), 1, F32, {}, [(0, 1030, 0, 1), (807, 200, 0, 1), (9, 1000, 0, 1), (1029, 1, 0, 1)]),
    # one per tile, two slices
    "f64-n300-nx9-nz72": ((300, 9, 72), 2, F64, {}, [(0, 300, 0, 2), (201, 80, 1, 1), (7, 290, 0, 1), (299, 1, 0, 2)]),
    # four slices: a diffusion workgroup per tile
    "f64-n130-nx8-nz200": ((130, 8, 200), 1, F64, {}, [(0, 130, 0, 1), (101, 20, 0, 1), (3, 120, 0, 1), (129, 1, 0, 1)]),
    # windowed: W tiles per instance
    "f64-n70-nx7-nz250-tall": ((70, 7, 250), 1, F64, dict(tall=True), [(0, 70, 0, 1), (45, 20, 0, 1), (3, 60, 0, 1), (69, 1, 0, 1)]),
}


# ---- D. arrays beyond 2^31 elements (fp32) and 2^32 bytes (fp64), assembled on the device from BIG_S distinct slabs
# along the slowest axis: slab t of the big array holds pattern t % BIG_S.  The sizes are chosen so that the slab that
# holds the element 2^31 (2^30, 2^29) elements before any element of slab t has ANOTHER pattern
# (tests/test_block_calls_geometry_cpu.py asserts it): a 32-bit offset cannot land on equal data.
BIG_S = 4
# f: a slab is one tracer of (ncrms, nx, nz); tracers per precision
BIG_F = {"shape": (502, 32, 64), "tracers": {F32: 1800, F64: 452}, "block": (3, 492)}
# u, w: a slab is a run of L levels; rho, adz and w repeat with the same period; slabs per precision (the last one has
# pattern 0 and is the top of the column: 1 modulo BIG_S)
BIG_UW = {"ncrms": 517, "nx": 32, "L": 64, "slabs": {F32: 1805, F64: 453}}


def slab_elems(kind):
    """elements of one slab of f / u / w"""
    if kind == "f":
        ncrms, nx, nz = BIG_F["shape"]
        return ncrms * (nx + 6) * (nz - 1)
    return BIG_UW["ncrms"] * (BIG_UW["nx"] + (5 if kind == "u" else 4)) * BIG_UW["L"]


def wrapped_patterns(t, elems, wrap):
    """the patterns of the slabs that hold the elements `wrap` elements before those of slab t (none before the array)"""
    d = wrap // elems
    return {(t - d - x) % BIG_S for x in (0, 1) if t - d - x >= 0 and (x == 0 or wrap % elems)}


def big_uw_inputs(dtype, seed):
    """the column of BIG_S + 1 slabs the truths of the big u, w come from: slabs 0 .. BIG_S - 1 and slab 0 again as the
    top of the column (its w has the level nz above it); the seven arrays of make_inputs, one tracer"""
    S, L = BIG_S, BIG_UW["L"]
    inp = make_inputs((BIG_UW["ncrms"], BIG_UW["nx"], (S + 1) * L + 1), 1, dtype, seed)
    for k in ("u", "w"):
        inp[k][:, :, S * L:(S + 1) * L] = inp[k][:, :, :L]
    for k in ("rho", "adz"):
        inp[k][:, S * L:(S + 1) * L] = inp[k][:, :L]
    return inp


# One wave-major fp64 plan whose f exceeds 2^32 bytes: the arrays repeat along the instance axis with `period` and f along
# the tracer axis with `S` patterns (tracer t holds pattern t % S); every call is independent per instance, so the truth
# repeats likewise.  The block and the tracer range reach past the 2^32-byte mark of the plan's f.
BIG_PLAN = {"shape": (8192, 32, 28), "T": 65, "period": 512, "S": 5, "block": (4001, 4100), "tracers": (60, 5)}


def wm_f_strides(shape):
    """(bytes of a tile, bytes of a tracer) of a wave-major fp64 plan's f (mpdata_plan.hip: tiles start on 128-byte lines, an
    odd number of lines apart)"""
    ncrms, nx, nz = shape
    slp = slp_of(nz)
    lines = ((nx + 6) * slp * (nz - 1) * 8 + 127) // 128
    lines += (lines & 1) == 0
    return lines * 128, (ncrms + slp - 1) // slp * lines * 128
