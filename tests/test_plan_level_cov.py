"""GPU tests of the per-level covariance of two tracers of a resident plan (include/mpdata_hip.h 3u):
mpdata_plan_level_cov_device, the host forms, the array forms, their Python face Plan.level_cov / level_cov_host /
level_cov, and the Fortran program tests/fortran/level_cov_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_cov_model.py: LC.level_cov on
the field the plan holds -- the plan model's (LC.PlanModelLevelCov: an EXACT plan's f is bit-identical to it) or, for FAST
plans, the plan's own whole export in front of the call.  ma and mb, where given, lie inside larger buffers with 4 KiB of
NaN on both sides, so a read outside the block's arrays poisons the result, and must come back unchanged; cov, mean_a and
mean_b are filled with NaN and lie between two patterned bands of 4 KiB, which must come back unchanged.  f is the
oracle's raw field moved by one half, so products and deviations take both signs.  Behind every call the whole export of f
and flux must equal the export taken in front of it, and a run behind the call must equal the model's run: the call
changed nothing, u and w included.

Before they touch the GPU, test_every_plan_kind and the block test assert ON THE MODEL, on the shape's uploaded field and
over the four pairs, that the central result differs in bits from the RAW result, from the result with the columns summed in
reverse order and from the one-pass formula in at least one output in ten (shapes with nx >= 3; at nx = 2 the reversed sum
is the same sum), and, at nx = 3, 11 and 17, from the result whose mean is formed with a rounded reciprocal in at least one
output in fifty: so a passing comparison tells these apart.

Plans have three tracers; the pairs are (0, 2), (2, 0), (1, 0) and (1, 1) -- non-adjacent, reversed (the negative stride
between the two streams), adjacent, and the variance (one stream).

Shapes (ncrms, nx, nz), the smallest at which a path of the kernel differs (NB = 8 columns in flight on each stream; the
kept form up to nx = 32, the re-read form above):
  (5, 3, 8)        padding slots of an 8-instance tile, one short batch
  (3, 8, 28)       exactly one batch
  (5, 11, 28)      two column batches, the last short
  (3, 17, 28)      three batches, the last of one column
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   63 elements; element 63 | 64 across two slices; three
                   and four slices with idle lanes and an idle wave
  (37, 3, 28), fp32 (74, 3, 28)   19 tiles: more than one thread block of four waves, the last partly filled
  (3, 32, 8), (3, 33, 8)   both precisions: the last nx of the kept form, the first of the re-read form
  fp32             pairs (even), the phantom (odd with the switch), the reference layout (odd without it)
  windowed plans   (nz > 238 with set_tall_columns): 239 and 300 levels, 18 instances, fp32 with 15 pseudo-instances (an
                   inner phantom); 250 levels without the switch is a reference-layout plan."""
import itertools

import numpy as np
import pytest

import fortran_records as FR
import level_cov_model as LC
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, nan_banded, nan_out, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
T = 3

# name -> (shape, tracers, dtype, switches)
KINDS = {
    "f64-nz8": ((5, 3, 8), T, F64, {}), "f64-nz28-nx8": ((3, 8, 28), T, F64, {}), "f64-nz28-nx11": ((5, 11, 28), T, F64, {}),
    "f64-nz28-nx17": ((3, 17, 28), T, F64, {}), "f64-nz64": ((3, 3, 64), T, F64, {}), "f64-nz65": ((3, 2, 65), T, F64, {}),
    "f64-nz72": ((3, 9, 72), T, F64, {}), "f64-nz140": ((2, 2, 140), T, F64, {}), "f64-nz238": ((2, 2, 238), T, F64, {}),
    "f64-nz28-5blocks": ((37, 3, 28), T, F64, {}), "f32-nz28-5blocks": ((74, 3, 28), T, F32, {}),
    "f64-nz8-nx32": ((3, 32, 8), T, F64, {}), "f64-nz8-nx33": ((3, 33, 8), T, F64, {}),
    "f32-nz8-nx32": ((3, 32, 8), T, F32, dict(odd=True)), "f32-nz8-nx33": ((3, 33, 8), T, F32, dict(odd=True)),
    "f32-nz28-even": ((6, 3, 28), T, F32, {}), "f32-nz72-even": ((4, 2, 72), T, F32, {}),
    "f32-nz28-odd": ((7, 3, 28), T, F32, dict(odd=True)), "f32-nz72-odd": ((3, 2, 72), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), T, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), T, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), T, F64, dict(tall=True)),
    "f64-nz239-tall-18": ((18, 2, 239), T, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), T, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant too; five kinds run a PERIODIC plan
FAST = ("f64-nz28-nx11", "f64-nz72", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall", "f64-nz8-nx33")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd", "f64-nz28-nx17")
PAIRS = ((0, 2), (2, 0), (1, 0), (1, 1))
HOWS = list(LC.MEANS)                                   # raw, central, ma, mb, both
SEED = 100

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = LC.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = LC.PlanModelLevelCov(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def assert_model_tells_the_variants_apart(F, name):
    """the conditions of the module's docstring on the field F (ncrms, nx+6, nzm, T), over the four pairs"""
    nx = F.shape[1] - 6
    d = {"raw": [], "rev": [], "one": [], "rec": []}
    for ta, tb in PAIRS:
        c = LC.level_cov(F, ta, tb)[0]
        d["raw"].append(LC.share_differs(c, LC.level_cov(F, ta, tb, raw=True)[0]))
        d["rev"].append(LC.share_differs(c, LC.level_cov(F, ta, tb, reverse=True)[0]))
        d["one"].append(LC.share_differs(c, LC.one_pass(F, ta, tb)))
        d["rec"].append(LC.share_differs(c, LC.level_cov(F, ta, tb, recip=True)[0]))
    s = {k: float(np.mean(v)) for k, v in d.items()}
    if nx >= 3:
        assert s["raw"] >= 0.1 and s["rev"] >= 0.1 and s["one"] >= 0.1, (name, s)
    if nx in (3, 11, 17):
        assert s["rec"] >= 0.02, (name, s)


def level_cov(M, p, name, ta, tb, how, k, sl0=0, n=None, means=(True, True), call=None):
    """Plan.level_cov on block [sl0, sl0 + n) with the profiles of kind `how` (seed k) -> (ma, mb, raw, cov, mean_a,
    mean_b), the outputs as host arrays (n, nzm) or None; means: which of mean_a, mean_b are asked for (never with RAW).
    The profiles and the bands are checked.  call: another callable with Plan.level_cov's arguments (a shard plan's)."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    ma, mb, raw = LC.call_args(n, nz, dt, k, how)
    sh = M.level_cov_shapes(n, nx, nz)
    ins = {key: nan_banded(a, sh[key]) for key, a in (("ma", ma), ("mb", mb)) if a is not None}
    orig = {key: r.clone() for key, (r, _) in ins.items()}
    outs = {"cov": nan_out(sh["cov"], dt)}
    for key, on in zip(("mean_a", "mean_b"), means):
        if on and not raw:
            outs[key] = nan_out(sh[key], dt)
    view = lambda key: ins[key][1] if key in ins else None
    out = lambda key: outs[key][2] if key in outs else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.level_cov)(ta, tb, out("cov"), view("ma"), view("mb"), LC.RAW if raw else 0, out("mean_a"), out("mean_b"), sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for key, (r, _) in ins.items():
        assert torch.equal(r.view(torch.uint8), orig[key].view(torch.uint8)), f"{key} changed"
    res = {}
    for key, (r, pristine, v) in outs.items():
        assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), f"{key}: a band byte changed"
        res[key] = to_host(v).reshape((n, nz - 1), order="F")
    return ma, mb, raw, res["cov"], res.get("mean_a"), res.get("mean_b")


def check(got, F, ta, tb, what, sl0=0, n=None):
    """the outputs of level_cov() against the model on block [sl0, sl0 + n) of the field F"""
    ma, mb, raw, cov, mean_a, mean_b = got
    n = F.shape[0] - sl0 if n is None else n
    want = LC.level_cov(np.asfortranarray(F[sl0:sl0 + n]), ta, tb, ma, mb, raw)
    assert_bitwise(cov, want[0], what + ": cov")
    if mean_a is not None:
        assert_bitwise(mean_a, want[1], what + ": mean_a")
    if mean_b is not None:
        assert_bitwise(mean_b, want[2], what + ": mean_b")


# ---- 1. every kind of plan: whole plan, every pair, every way the means come about, with and without the mean outputs;
# behind the upload and behind a run (a windowed plan's seams and a periodic plan's halos are stale); a run behind the calls
MEAN_OUTS = ((True, True), (False, False), (True, False), (False, True))


@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T) and (F0 < 0).any() and (F0 > 0).any()
    assert_model_tells_the_variants_apart(F0, name)
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    k = 0
    for state in ("upload", "run", "run 2"):
        if state != "upload":
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} {state}: in front of the calls")
        F = m.a["f"]
        # every pair with every way of the means; the mean outputs rotate (behind the upload: all four combinations of them)
        combos = list(itertools.product(PAIRS, HOWS))
        if state == "run 2":
            combos = combos[::3]
        for j, ((ta, tb), how) in enumerate(combos):
            for means in (MEAN_OUTS if state == "upload" and how != "raw" and (ta, tb) in ((2, 0), (1, 1)) else (MEAN_OUTS[j % 4],)):
                k += 1
                got = level_cov(M, p, name, ta, tb, how, 300 + k, means=means)
                check(got, F, ta, tb, f"{name} {state} pair {ta, tb} {how} means {means}")
        same(whole(M, p, name), before, f"{name} {state}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()
    if name in FAST:
        # FAST: the same bits as EXACT on the uploaded f; after a run against the plan's own export
        p = new_plan(M, name, variant=M.VARIANT_FAST)
        upload(p, inp)
        for state in ("upload", "run"):
            if state == "run":
                p.run()
            before = whole(M, p, name)
            if state == "upload":
                assert_bitwise(before["f"], F0, f"{name} FAST: the uploaded f")
            for j, ((ta, tb), how) in enumerate(itertools.product(PAIRS, HOWS)):
                got = level_cov(M, p, name, ta, tb, how, 400 + j, means=MEAN_OUTS[j % 4])
                check(got, before["f"], ta, tb, f"{name} FAST {state} pair {ta, tb} {how}")
            same(whole(M, p, name), before, f"{name} FAST {state}: behind the calls")
        p.close()


# ---- 2. blocks: only the block's instances reach the outputs, and nothing else is written
BLOCKS = {
    # eight instances per tile, five instances: inside the tile, one instance, the last one
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    # two per tile: mid-tile to mid-tile, the last (half-filled) tile
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    # 19 tiles in five thread blocks: a block of instances across thread blocks, odd ends, the last instance alone
    "f64-nz28-5blocks": [(7, 11), (3, 32), (36, 1), (8, 8)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    "f64-nz8-nx33": [(1, 2), (2, 1)],
    # fp32 pairs: a block that splits pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    "f32-nz28-5blocks": [(15, 19), (1, 72), (73, 1)],
    # fp32 pairs, odd plan of 7 (instance 6 shares its pair with the phantom): blocks that hold and miss instance 6, the
    # single-instance block of instance 6 among them
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz8-nx32": [(1, 2), (2, 1), (0, 1)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    # windowed plans: behind an import (the first) and behind a run (the others: stale seams), a block and the whole
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-18": [(15, 3), (17, 1), (1, 16)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_reach_only_their_outputs(mpdata, oracle, name):
    """the pairs and the ways of the means rotate over the blocks, each block with three calls; a run between the blocks"""
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    assert_model_tells_the_variants_apart(inputs(oracle, name)["f"], name)
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for b, (sl0, n) in enumerate(BLOCKS[name]):
        if b:
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} block {sl0, n}: in front of the calls")
        for j in range(3):
            ta, tb = PAIRS[(b + j) % 4]
            how = HOWS[(2 * b + j) % 5]
            got = level_cov(M, p, name, ta, tb, how, 500 + 10 * b + j, sl0, n, means=MEAN_OUTS[(b + j) % 4])
            check(got, m.a["f"], ta, tb, f"{name} block {sl0, n} pair {ta, tb} {how}", sl0, n)
        same(whole(M, p, name), before, f"{name} block {sl0, n}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()


# ---- 3. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall", "f32-nz8-nx33"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, pair, how, mean outputs)
    script = ((0, ncrms, (0, 2), "central", (True, True)), (1, ncrms - 1, (2, 0), "ma", (False, True)), (ncrms - 1, 1, (1, 1), "raw", (False, False)),
              (0, 2, (1, 0), "both", (True, False)), (0, ncrms, (1, 1), "mb", (True, True)))
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    p.run()
    assert m.run() is None
    before = whole(M, p, name)
    for k, (sl0, n, (ta, tb), how, means) in enumerate(script):
        ma, mb, raw = LC.call_args(n, nz, dt, 600 + k, how)
        keep = [None if x is None else np.array(x, order="F") for x in (ma, mb)]
        cov, mean_a, mean_b = (np.full((n, nz - 1), np.nan, dt, order="F") if on else None for on in (True,) + means)
        p.level_cov_host(ta, tb, cov, ma, mb, LC.RAW if raw else 0, mean_a, mean_b, sl0, n)
        for x, kx, nm in zip((ma, mb), keep, ("ma", "mb")):
            if x is not None:
                assert_bitwise(x, kx, f"{name} host {sl0, n}: {nm}")
        check((ma, mb, raw, cov, mean_a, mean_b), m.a["f"], ta, tb, f"{name} host form {sl0, n} pair {ta, tb} {how}", sl0, n)
        same(whole(M, p, name), before, f"{name} host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.level_cov_host(0, 2, cov[:, :-1], sl0=0, n=ncrms)      # a wrong shape
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name} host form: a run behind the calls")
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 1, 70000): the second trip over
# gridDim.y.  f is random, so instance b differs from b - 256 and level k from k - 65535.  Each with a block inside the
# arrays (sl0 > 0).
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 1, 70000), 3, (1, 1)),
          "nx33": ((5, 33, 4), 3, (2, 2))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr])
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (ncrms, nx + 6, nz - 1, ntr)).astype(dt))
    fd = to_dev(f)
    calls = (((0, ncrms), (0, ntr - 1), "central", (True, True)), ((b0, bn), (ntr - 1, 1), "ma", (False, True)),
             ((b0, bn), (1, 1), "raw", (False, False)), ((0, ncrms), (1, 0), "both", (True, False)), ((b0, bn), (0, 0), "mb", (True, True)))
    for k, ((sl0, n), (ta, tb), how, means) in enumerate(calls):
        ma, mb, raw = LC.call_args(n, nz, dt, 700 + k, how)
        want = LC.level_cov(np.asfortranarray(f[sl0:sl0 + n]), ta, tb, ma, mb, raw)
        # (nx = 1: a formed mean is the cell itself, so its deviation and with it cov is zero; the given profiles, RAW and
        # the mean outputs still tell instances and levels apart)
        assert want[0].any() or (nx == 1 and how not in ("raw", "both"))
        for w in want:
            if w is not None and w.any():
                assert n <= 256 or not np.array_equal(w[256:], w[:n - 256])
                assert nz - 1 <= 65535 or not np.array_equal(w[:, 65535:], w[:, :nz - 1 - 65535])
        sh = M.level_cov_shapes(n, nx, nz)
        ins = {key: nan_banded(a, sh[key]) for key, a in (("ma", ma), ("mb", mb)) if a is not None}
        orig = {key: r.clone() for key, (r, _) in ins.items()}
        outs = {"cov": nan_out(sh["cov"], dt)}
        for key, on in zip(("mean_a", "mean_b"), means):
            if on:
                outs[key] = nan_out(sh[key], dt)
        view = lambda key: ins[key][1] if key in ins else None
        out = lambda key: outs[key][2] if key in outs else None
        torch.cuda.synchronize()
        M.level_cov(fd, ta, tb, out("cov"), view("ma"), view("mb"), LC.RAW if raw else 0, out("mean_a"), out("mean_b"), sl0, n)
        torch.cuda.synchronize()
        for key, (r, _) in ins.items():
            assert torch.equal(r.view(torch.uint8), orig[key].view(torch.uint8)), f"{key} changed"
        for key, w in zip(("cov", "mean_a", "mean_b"), want):
            if key in outs:
                r, pristine, v = outs[key]
                assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), key
                assert_bitwise(to_host(v), w, f"array form {case} block {sl0, n} pair {ta, tb} {how}: {key}")
        assert_bitwise(to_host(fd), f, f"array form {case}: f is only read")


# ---- 4. every error code, in the stated order; the plan's state before and after
def test_errors_change_nothing(mpdata, oracle):
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    import torch
    buf = lambda: torch.full((nz - 1, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    cov, w = buf(), to_dev(LC.make_profile(ncrms, nz, dt, 530))

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.level_cov, 0, 2, cov) == M.ESTATE                              # never filled
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    one = w.data_ptr()
    raw = lambda sl0=0, n=ncrms, ta=0, tb=2, ma=None, mb=None, mode=0, c=cov.data_ptr(), mean_a=None, mean_b=None: \
        L.mpdata_plan_level_cov_device(p._p, sl0, n, ta, tb, ma, mb, mode, c, mean_a, mean_b)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for ta, tb in ((-1, 0), (0, -1), (3, 0), (0, 3), (3, 3)):
        assert raw(ta=ta, tb=tb) == M.EINVAL and b"tracer pair" in err(), (ta, tb)
    for mode in (2, 3, 4, -2):
        assert raw(mode=mode) == M.EINVAL and b"mode bits" in err(), mode
    for k in ("ma", "mb", "mean_a", "mean_b"):
        assert raw(mode=1, **{k: one}) == M.EINVAL and b"non-null " + k.encode() in err(), k
    assert raw(c=None) == M.EINVAL and b"null cov" in err()
    # the order: the range, the pair, the mode bits, RAW with a profile, cov
    assert raw(0, 0, 9, 9, one, None, 3, None) == M.EINVAL and b"n = 0" in err()
    assert raw(ta=9, ma=one, mode=3, c=None) == M.EINVAL and b"tracer pair" in err()
    assert raw(ma=one, mode=3, c=None) == M.EINVAL and b"mode bits" in err()
    assert raw(ma=one, mode=1, c=None) == M.EINVAL and b"non-null ma" in err()
    # a host form of the other precision; its arguments come first
    c32 = np.full((ncrms, nz - 1), np.nan, F32, order="F")
    h32 = lambda ta=0, tb=2, mode=0, c=c32.ctypes.data, ma=None: L.mpdata_plan_level_cov_f32(p._p, 0, ncrms, ta, tb, ma, None, mode, c, None, None)
    assert h32() == M.ESTATE
    assert h32(c=None) == M.EINVAL and b"null cov" in err()
    assert h32(tb=3) == M.EINVAL and h32(mode=2) == M.EINVAL and h32(mode=1, ma=c32.ctypes.data) == M.EINVAL
    assert np.isnan(c32).all()
    # the array forms: sizes, the block, f, then the pair, the mode bits, RAW with a profile, cov
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=8, ta=0, tb=2, ma=None, mode=0, c=8: \
        L.mpdata_level_cov_device(ncrms, 5, nz, 3, sl0, n, f, ta, tb, ma, None, mode, c, None, None, None)
    assert arr(nz=1, sl0=2, n=3, f=None, c=None) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, c=None) == M.EINVAL and b"outside" in err()
    assert arr(f=None, ta=3, c=None) == M.EINVAL and b"null f" in err()
    assert arr(ta=3, mode=2, c=None) == M.EINVAL and b"tracer pair" in err()
    assert arr(mode=2, c=None) == M.EINVAL and b"mode bits" in err()
    assert arr(mode=1, ma=8, c=None) == M.EINVAL and b"non-null ma" in err()
    assert arr(c=None) == M.EINVAL and b"null cov" in err()
    torch.cuda.synchronize()
    assert torch.isnan(cov).all()                                                # no refused call wrote an output
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    p.level_cov(0, 2, cov)                                                       # ... and the plan still works
    p.sync()
    assert_bitwise(to_host(cov), LC.level_cov(inp["f"], 0, 2)[0], "the call behind the refused ones")
    p.close()


# ---- 5. a multi-GPU handle is refused; the single-device plans of its shards take the call
def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    import torch
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    p = M.Plan(*shape, ntr, dtype=dt, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name)
    cov = torch.full((nz - 1, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    with pytest.raises(M.MpdataError) as e:
        p.level_cov(0, 2, cov)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.level_cov_host(0, 2, np.zeros((ncrms, nz - 1), dt, order="F"))
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.level_cov(9, 9, cov)                               # (the handle comes before the pair)
    assert e.value.code == M.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(cov).all()
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        for j, how in enumerate(("central", "ma", "raw")):
            ta, tb = PAIRS[(g + j) % 4]
            got = level_cov(M, q, name, ta, tb, how, 800 + 10 * g + j, 0, nloc, call=q.level_cov)
            check(got, m.a["f"], ta, tb, f"shard {g} pair {ta, tb} {how}", s0, nloc)
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 6. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (ta, tb)
FORTRAN = {
    "f64": (F64, "level_cov_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "level_cov_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f64-whole": (F64, "level_cov_calls", (5, 3, 28), (0, 5), (1, 0)), "f32-odd-ref": (F32, "level_cov_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "level_cov_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "level_cov_calls_sp", (4, 2, 72), (1, 2), (1, 1)),
    "f64-nx33": (F64, "level_cov_calls", (3, 33, 8), (1, 2), (0, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: (ta, tb) on the block with both means formed and returned; (tb, ta) on the whole plan about a
    given ma, mean_b returned; the RAW second moment of ta; a RAW call with a profile, refused"""
    dt, exe, shape, (sl0, n), (ta, tb) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = LC.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    ma_b = LC.make_profile(ncrms, nz, dt, 900)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, ta, tb], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("ma_b", ma_b)]
    # the replay on the model
    m = LC.PlanModelLevelCov(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    cov_a, mean_a_a, mean_b_a = m.level_cov(ta, tb, sl0=sl0, n=n, mean_a=True, mean_b=True)
    rc("cov_block"); rc("sync")
    want += [("cov_a", cov_a), ("mean_a_a", mean_a_a), ("mean_b_a", mean_b_a)]
    cov_b, _, mean_b_b = m.level_cov(tb, ta, ma_b, mean_b=True)
    rc("cov_given"); rc("sync")
    want += [("cov_b", cov_b), ("mean_b_b", mean_b_b)]
    cov_c, _, _ = m.level_cov(ta, ta, mode=LC.RAW)
    rc("cov_raw"); rc("sync")
    want += [("cov_c", cov_c)]
    rc("cov_refused", m.level_cov(ta, tb, ma_b, mode=LC.RAW))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
