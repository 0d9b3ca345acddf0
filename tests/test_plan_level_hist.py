"""GPU tests of the per-level histograms of a resident plan's tracers (include/mpdata_hip.h 3ab):
mpdata_plan_level_hist_device, the host forms, the array forms, their Python face Plan.level_hist / level_hist_host /
level_hist, and the Fortran program tests/fortran/level_hist_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_hist_model.py: LH.level_hist on
the field the plan holds -- the plan model's (LH.PlanModelLevelHist: an EXACT plan's f is bit-identical to it) or, for FAST
plans, the plan's own whole export in front of the call.  cnt and bsum are filled with NaN and lie between two patterned
bands of 4 KiB, which must come back unchanged.  Behind every call the whole export of f and flux must equal the export
taken in front of it, and a run behind the calls must equal the model's run: the call changed nothing.  On one kind per
family the outputs are also held against the existing Plan.level_cond called bin by bin on the same plan (lo = e_j, hi =
e_{j+1}): an oracle that does not pass through the new model.

Behind the upload every fourth cell of the field is a multiple of 1/8 and the edges lie on multiples of 1/4 or 1/8
(LH.call_edges), so c == e_j occurs in most rows; behind a run the edges are a sorted sample of the field's own values
(LH.sample_edges).  tests/test_level_hist_cpu.py asserts on the model, for every shape and bin count below, that >= for >,
a bin index off by one, the edge of the wrong bin, a reversed walk, a mask multiplied in and a NaN counted in bin 0 each
change at least one output row in ten.

Plans have three tracers; the (tc; first, ntr) triples are (0; 0, 3), (2; 0, 2), (1; 1, 1) and (1; 2, 1) -- tc inside the
range, above it, equal to the only value tracer, and below the only one.  The outputs are cnt and bsum, cnt alone, bsum
alone.

The bin counts NBS: 1, 2 and 32, and the value on each side of every boundary the kernel has -- the bin classes of a walk
(4 | 5, 8 | 9; fp64 also 16 | 17) and the bin groups of a call (fp64: 16 bins a walk, so 16 | 17 and 32 = two full groups;
fp32: 8 bins a walk, so 8 | 9, 16 | 17, 24 | 25 and 32 = four groups; the reference layout: 8 a walk in both precisions).
The kernel has no index cache, hence no limit on nx of its own.

Shapes (ncrms, nx, nz), the smallest at which a path of the walk differs (NB = 8 columns in flight), from 3v's list:
  (5, 3, 8)        padding slots of an 8-instance tile, one short batch
  (3, 8, 28)       exactly one batch
  (5, 11, 28), (3, 17, 28)   short last batches
  (3, 3, 64), (3, 2, 65), (3, 9, 72), (2, 2, 140), (2, 2, 238)   slices
  (37, 3, 28), fp32 (74, 3, 28)   19 tiles: more than one thread block of four waves, the last partly filled
  fp32             pairs (even), the phantom (odd with the switch), the reference layout (odd without it)
  reference layout (5, 3, 12), (6, 3, 12), (7, 3, 12), (2, 3, 250)
  windowed plans   239 and 300 levels, 18 instances, fp32 with an inner phantom."""
import numpy as np
import pytest

import fortran_records as FR
import level_hist_model as LH
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, nan_out, upload
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
    "f32-nz28-even": ((6, 3, 28), T, F32, {}), "f32-nz28-odd": ((7, 3, 28), T, F32, dict(odd=True)),
    "f32-nz72-odd": ((3, 2, 72), T, F32, dict(odd=True)),
    "f64-nz12-ref": ((5, 3, 12), T, F64, dict(ref=True)), "f32-nz12-ref": ((6, 3, 12), T, F32, dict(ref=True)),
    "f32-nz12-odd-ref": ((7, 3, 12), T, F32, {}),      # (an odd fp32 plan without the switch keeps the reference layout)
    "f64-nz250-ref": ((2, 3, 250), T, F64, {}),        # (above 238 levels without the switch: the reference layout)
    "f64-nz239-tall": ((2, 3, 239), T, F64, dict(tall=True)), "f64-nz300-tall": ((3, 2, 300), T, F64, dict(tall=True)),
    "f64-nz239-tall-18": ((18, 2, 239), T, F64, dict(tall=True)),
    "f32-nz239-tall-odd": ((3, 2, 239), T, F32, dict(tall=True, odd=True)),
}
REF = ("f32-nz12-odd-ref", "f64-nz12-ref", "f32-nz12-ref", "f64-nz250-ref")
# one kind of each family runs the FAST variant, a PERIODIC plan and the cross-check against level_cond
FAST = ("f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall")
PERIODIC = ("f64-nz28-nx11", "f32-nz72-odd", "f64-nz12-ref", "f32-nz239-tall-odd")
CROSS = ("f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f32-nz239-tall-odd")
TRIPLES = ((0, 0, 3), (2, 0, 2), (1, 1, 1), (1, 2, 1))      # (tc, first, ntr)
OUTS = ("both", "cnt", "bsum")
NBS = (1, 2, 4, 5, 8, 9, 16, 17, 24, 25, 32)
SEED = 100

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = LH.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = LH.PlanModelLevelHist(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def level_hist(M, p, name, triple, edges, nb, outs, sl0=0, n=None, call=None):
    """Plan.level_hist on block [sl0, sl0 + n) with the outputs `outs` -> (cnt, bsum) as host arrays (n, nzm, nb) and (n,
    nzm, nb, ntr) or None.  The bands are checked.  call: another callable with Plan.level_hist's arguments."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    tc, first, ntr = triple
    sh = M.level_hist_shapes(n, nx, nz, nb, ntr)
    bufs = {key: nan_out(sh[key], dt) for key in ("cnt", "bsum") if outs in ("both", key)}
    out = lambda key: bufs[key][2] if key in bufs else None
    keep = np.array(edges)
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.level_hist)(tc, edges, out("cnt"), out("bsum"), first, nb, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    assert_bitwise(np.asarray(edges), keep, "edges")
    res = {}
    for key, (r, pristine, v) in bufs.items():
        assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), f"{key}: a band byte changed"
        res[key] = to_host(v)
    return res.get("cnt"), res.get("bsum")


def check(got, F, triple, edges, nb, what, sl0=0, n=None):
    """the outputs of level_hist() against the model on block [sl0, sl0 + n) of the field F"""
    cnt, bsum = got
    tc, first, ntr = triple
    n = F.shape[0] - sl0 if n is None else n
    want = LH.level_hist(np.asfortranarray(F[sl0:sl0 + n]), tc, edges, nb, first, ntr)
    assert cnt is not None or bsum is not None
    if cnt is not None:
        assert_bitwise(cnt, want[0], what + ": cnt")
    if bsum is not None:
        assert_bitwise(bsum, want[1], what + ": bsum")


# ---- 1. every kind of plan: whole plan, every triple, the bin counts and the output sets rotating so that every bin count
# meets every kind; behind the upload (ties on the grid) and behind a run (edges sampled from the field; a windowed plan's
# seams and a periodic plan's halos are stale); a run behind the calls
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0 = inp["f"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T) and (F0 < 0).any() and (F0 > 0).any()
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inp)
    if name in PERIODIC:
        p.set_boundary(M.BOUNDARY_PERIODIC)
        assert m.set_boundary(PM.PERIODIC) is None
    k = 0
    for state in ("upload", "run"):
        if state != "upload":
            p.run()
            assert m.run() is None
        before = whole(M, p, name)
        same(before, snap(m), f"{name} {state}: in front of the calls")
        F = m.a["f"]
        for j, nb in enumerate(NBS if state == "upload" else NBS[::2]):
            triple = TRIPLES[(j + (state == "run")) % 4]
            outs = OUTS[(j + j // 3) % 3]
            k += 1
            edges = LH.call_edges(nb, k) if state == "upload" else LH.sample_edges(F, triple[0], nb, 300 + k)
            got = level_hist(M, p, name, triple, edges, nb, outs)
            check(got, F, triple, edges, nb, f"{name} {state} triple {triple} nb {nb} outputs {outs}")
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
            for j, nb in enumerate(NBS[1::2]):
                triple = TRIPLES[j % 4]
                edges = LH.call_edges(nb, 40 + j) if state == "upload" else LH.sample_edges(before["f"], triple[0], nb, 400 + j)
                got = level_hist(M, p, name, triple, edges, nb, OUTS[j % 3])
                check(got, before["f"], triple, edges, nb, f"{name} FAST {state} triple {triple} nb {nb}")
            same(whole(M, p, name), before, f"{name} FAST {state}: behind the calls")
        p.close()


# ---- 2. the existing level_cond, bin by bin on the same plan: cnt(:,:,j), bsum(:,:,j,:) have the bits of its cnt and csum
# with lo = e_j, hi = e_{j+1}
@pytest.mark.parametrize("name", CROSS)
def test_bins_have_the_bits_of_level_cond(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    tdt = torch.float64 if dt == F64 else torch.float32
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for state in ("upload", "run"):
        if state == "run":
            p.run()
        F = whole(M, p, name, ("f",))["f"]
        for j, nb in enumerate((2, 9, 17)):
            tc, first, ntr_ = TRIPLES[j]
            edges = LH.call_edges(nb, 4 * j) if state == "upload" else LH.sample_edges(F, tc, nb, 450 + j)   # (finite ends)
            cnt, bsum = level_hist(M, p, name, (tc, first, ntr_), edges, nb, "both")
            sh = M.level_cond_shapes(ncrms, nx, nz, ntr_)
            for b in range(nb):
                lo = torch.full(sh["lo"], float(dt(edges[b])), dtype=tdt, device="cuda:0")
                hi = torch.full(sh["hi"], float(dt(edges[b + 1])), dtype=tdt, device="cuda:0")
                c1 = torch.full(sh["cnt"], float("nan"), dtype=tdt, device="cuda:0")
                s1 = torch.full(sh["csum"], float("nan"), dtype=tdt, device="cuda:0")
                torch.cuda.synchronize()
                p.level_cond(tc, lo, hi, c1, s1, first)
                p.sync()
                assert_bitwise(cnt[:, :, b], to_host(c1), f"{name} {state} nb {nb} bin {b}: cnt against level_cond")
                assert_bitwise(bsum[:, :, b, :], to_host(s1), f"{name} {state} nb {nb} bin {b}: bsum against level_cond")
    p.close()


# ---- 3. blocks: only the block's instances reach the outputs, and nothing else is written
BLOCKS = {
    "f64-nz8": [(1, 3), (2, 1), (4, 1), (0, 5)],
    "f64-nz28-nx11": [(1, 3), (4, 1), (0, 4)],
    "f64-nz28-5blocks": [(7, 11), (3, 32), (36, 1), (8, 8)],
    "f64-nz72": [(1, 1), (1, 2)],
    "f64-nz140": [(1, 1), (0, 1)],
    # fp32 pairs: blocks that start at an odd instance and split pairs at both ends
    "f32-nz28-even": [(1, 3), (5, 1), (2, 2)],
    "f32-nz28-5blocks": [(15, 19), (1, 72), (73, 1)],
    "f32-nz28-odd": [(1, 2), (6, 1), (5, 2), (0, 6), (3, 3), (0, 7)],
    "f32-nz72-odd": [(2, 1), (1, 1), (0, 2)],
    "f32-nz12-odd-ref": [(1, 3), (6, 1)],
    "f64-nz12-ref": [(1, 3), (4, 1)],
    "f64-nz239-tall": [(1, 1), (0, 1), (0, 2)],
    "f64-nz239-tall-18": [(15, 3), (17, 1), (1, 16)],
    "f32-nz239-tall-odd": [(1, 1), (2, 1), (0, 2), (0, 3)],
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_reach_only_their_outputs(mpdata, oracle, name):
    """the triples, the bin counts and the output sets rotate over the blocks, each block with three calls; a run between
    the blocks"""
    M = mpdata
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
            triple, nb, outs = TRIPLES[(b + j) % 4], NBS[(4 * b + 3 * j + 2) % len(NBS)], OUTS[(b + 2 * j) % 3]
            F = m.a["f"]
            edges = LH.call_edges(nb, 10 * b + j) if b == 0 else LH.sample_edges(F[sl0:sl0 + n], triple[0], nb, 500 + 10 * b + j)
            got = level_hist(M, p, name, triple, edges, nb, outs, sl0, n)
            check(got, F, triple, edges, nb, f"{name} block {sl0, n} triple {triple} nb {nb} outputs {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} block {sl0, n}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()


# ---- 4. selection means selection: +inf and NaN in every EXCLUDED cell of a value tracer never reach bsum; a NaN in the
# binned tracer is in no bin
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref"])
def test_excluded_cells_and_nans_reach_no_bin(mpdata, oracle, name):
    M = mpdata
    F0 = inputs(oracle, name)["f"]
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    for tc, t, nb in ((0, 2, 5), (2, 1, 17), (1, 0, 32)):
        edges = np.clip(LH.call_edges(nb, 0), -0.5, 1.5)       # (columns below and above every bin)
        P = LH.plant(F0, tc, edges, nb, t)
        assert np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        want = LH.level_hist(P, tc, edges, nb, 0, T)[1]
        assert np.isfinite(want).all()
        assert np.mean(~np.isfinite(LH.level_hist(P, tc, edges, nb, t, 1, multiply=True)[1])) >= 0.1
        p.import_device(f=to_dev(np.asfortranarray(P[..., t])), first_tracer=t)
        for triple in ((tc, 0, T), (tc, t, 1)):
            got = level_hist(M, p, name, triple, edges, nb, "both")
            assert np.isfinite(got[1]).all()
            check(got, P, triple, edges, nb, f"{name} planted tracer {t} under tc {tc} nb {nb} triple {triple}")
        p.import_device(f=to_dev(np.asfortranarray(F0[..., t])), first_tracer=t)
        # NaNs in the binned tracer itself, also as a value
        N = LH.plant_nan(F0, tc)
        p.import_device(f=to_dev(np.asfortranarray(N[..., tc])), first_tracer=tc)
        e2 = LH.call_edges(nb, 3)                                  # -inf and +inf ends: everything but the NaNs
        got = level_hist(M, p, name, (tc, t, 1), e2, nb, "both")
        assert got[0].sum(axis=2).min() < N.shape[1] - 6 and np.isfinite(got[1]).all()
        check(got, N, (tc, t, 1), e2, nb, f"{name} NaN in tc {tc} nb {nb}")
        p.import_device(f=to_dev(np.asfortranarray(F0[..., tc])), first_tracer=tc)
    p.close()


# ---- 5. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, tc, nb, outputs): all tracers
    script = ((0, ncrms, 0, 5, "both"), (1, ncrms - 1, 2, 17, "bsum"), (ncrms - 1, 1, 1, 32, "cnt"), (0, 2, 1, 1, "bsum"),
              (0, ncrms, 2, 9, "both"))
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    p.run()
    assert m.run() is None
    before = whole(M, p, name)
    for k, (sl0, n, tc, nb, outs) in enumerate(script):
        edges = LH.sample_edges(m.a["f"][sl0:sl0 + n], tc, nb, 600 + k)
        cnt = np.full((n, nz - 1, nb), np.nan, dt, order="F") if outs != "bsum" else None
        bsum = np.full((n, nz - 1, nb, T), np.nan, dt, order="F") if outs != "cnt" else None
        p.level_hist_host(tc, edges, cnt, bsum, nb, sl0, n)
        check((cnt, bsum), m.a["f"], (tc, 0, T), edges, nb, f"{name} host form {sl0, n} tc {tc} nb {nb} {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.level_hist_host(0, edges, cnt[:, :-1], None, nb, 0, ncrms)      # a wrong shape
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name} host form: a run behind the calls")
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 3, 70000): the second trip over
# gridDim.y.  Each with a block inside the arrays (sl0 > 0).  The last call plants +inf and NaN in the excluded cells.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 3, 70000), 3, (1, 1)),
          "nx17": ((5, 17, 4), 3, (2, 2))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr_all, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([77, ncrms, ntr_all])
    f = rng.uniform(-1, 2, (ncrms, nx + 6, nz - 1, ntr_all))
    f = np.asfortranarray(np.where(rng.integers(0, 2, f.shape) == 0, np.round(f * 8) / 8, f).astype(dt))
    # ((sl0, n), (tc, first, ntr), nb, outputs, planted tracer or None)
    calls = (((0, ncrms), (0, 0, ntr_all), 8, "both", None), ((b0, bn), (ntr_all - 1, 0, 2), 9, "bsum", None),
             ((b0, bn), (1, 1, 1), 32, "both", None), ((0, ncrms), (1, 0, 1), 1, "cnt", None), ((b0, bn), (1, 2, 1), 17, "both", 2))
    if case == "rows70000":
        calls = calls[1:3] + calls[4:]
    for k, ((sl0, n), (tc, first, ntr), nb, outs, planted) in enumerate(calls):
        fb = np.asfortranarray(f[sl0:sl0 + n])
        edges = LH.call_edges(nb, 4 * k)
        g = f
        if planted is not None:
            g = np.array(f, order="F")
            edges = np.clip(edges, -0.5, 1.5)
            g[sl0:sl0 + n] = LH.plant(fb, tc, edges, nb, planted)
            assert not np.isfinite(g[..., planted]).all()
        fd = to_dev(g)
        want = LH.level_hist(np.asfortranarray(g[sl0:sl0 + n]), tc, edges, nb, first, ntr)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and want[0].any() and want[1].any()
        sh = M.level_hist_shapes(n, nx, nz, nb, ntr)
        bufs = {key: nan_out(sh[key], dt) for key in ("cnt", "bsum") if outs in ("both", key)}
        out = lambda key: bufs[key][2] if key in bufs else None
        torch.cuda.synchronize()
        M.level_hist(fd, tc, edges, out("cnt"), out("bsum"), first, nb, sl0, n)
        torch.cuda.synchronize()
        for key, w in zip(("cnt", "bsum"), want):
            if key in bufs:
                r, pristine, v = bufs[key]
                assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), key
                assert_bitwise(to_host(v), w, f"array form {case} block {sl0, n} triple {tc, first, ntr} nb {nb}: {key}")
        assert_bitwise(to_host(fd), g, f"array form {case}: f is only read")


# ---- 6. every error code, in the stated order; the plan's state before and after; every refusal leaves the outputs NaN
def test_errors_change_nothing(mpdata, oracle):
    import ctypes
    import torch
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    NB = 5
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda:0")
    cnt, bsum = nan(NB, nz - 1, ncrms), nan(T, NB, nz - 1, ncrms)
    e_h = LH.call_edges(NB, 0)
    arr_of = lambda a: (ctypes.c_double * len(a))(*a)
    e_ok, e_nan, e_desc = arr_of(e_h), arr_of([0, float("nan"), 1, 2, 3, 4]), arr_of([0, 1, 3, 2, 4, 5])
    E = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.level_hist, 0, e_h, cnt, bsum) == M.ESTATE                     # never filled
    assert code(p.level_hist, 3, e_h, cnt, bsum) == M.EINVAL                     # ... the arguments come first
    upload(p, inp)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    raw = lambda sl0=0, n=ncrms, tc=0, nb=NB, e=E(e_ok), c=cnt.data_ptr(), s=bsum.data_ptr(), first=0, ntr=T: \
        L.mpdata_plan_level_hist_device(p._p, sl0, n, tc, nb, e, c, s, first, ntr)
    assert raw(0, ncrms, 0, NB, E(e_ok), cnt.data_ptr(), None, 0, 0) in (0,)     # (the lambda itself is right)
    p.sync()
    cnt.fill_(float("nan"))
    assert L.mpdata_plan_level_hist_device(None, 0, ncrms, 0, NB, E(e_ok), cnt.data_ptr(), bsum.data_ptr(), 0, T) == M.EINVAL
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for tc in (-1, 3, 9):
        assert raw(tc=tc) == M.EINVAL and b"binned tracer" in err(), tc
    for nb in (0, -1, 33):
        assert raw(nb=nb) == M.EINVAL and b"nb" in err(), nb
    assert raw(e=None) == M.EINVAL and b"null edges" in err()
    assert raw(e=E(e_nan)) == M.EINVAL and b"NaN" in err()
    assert raw(e=E(e_desc)) == M.EINVAL and b"edges[2] > edges[3]" in err()
    assert raw(c=None, s=None) == M.EINVAL and b"cnt and bsum are both NULL" in err()
    for first, n_ in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raw(first=first, ntr=n_) == M.EINVAL and b"tracer range" in err(), (first, n_)
    # the order: the range, tc, nb, the edges, the outputs, the tracers
    assert raw(0, 0, 9, 0, None, None, None, 9, 9) == M.EINVAL and b"n = 0" in err()
    assert raw(tc=9, nb=0, e=None, c=None, s=None, first=9) == M.EINVAL and b"binned tracer" in err()
    assert raw(nb=0, e=None, c=None, s=None, first=9) == M.EINVAL and b"nb 0" in err()
    assert raw(e=None, c=None, s=None, first=9) == M.EINVAL and b"null edges" in err()
    assert raw(e=E(e_nan), c=None, s=None, first=9) == M.EINVAL and b"NaN" in err()
    assert raw(c=None, s=None, first=9) == M.EINVAL and b"cnt and bsum" in err()
    assert raw(c=None, first=9) == M.EINVAL and b"tracer range" in err()
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all() and torch.isnan(bsum).all()                    # no refused call wrote an output
    # a host form of the other precision; its arguments come first
    c32 = np.full((ncrms, nz - 1, NB), np.nan, F32, order="F")
    h32 = lambda tc=0, e=E(e_ok), c=c32.ctypes.data: L.mpdata_plan_level_hist_f32(p._p, 0, ncrms, tc, NB, e, c, None)
    assert h32() == M.ESTATE
    assert h32(c=None) == M.EINVAL and b"cnt and bsum" in err()
    assert h32(tc=3) == M.EINVAL and h32(e=None) == M.EINVAL
    assert np.isnan(c32).all()
    # the array forms: sizes, the block, f, then tc, nb, the edges, the outputs, the tracers
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=8, tc=0, nb=NB, e=E(e_ok), c=8, s=8, first=0, ntr=3: \
        L.mpdata_level_hist_device(ncrms, 5, nz, 3, sl0, n, f, tc, nb, e, c, s, first, ntr, None)
    assert arr(nz=1, sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, f=None, tc=3) == M.EINVAL and b"outside" in err()
    assert arr(f=None, tc=3) == M.EINVAL and b"null f" in err()
    assert arr(tc=3, nb=0) == M.EINVAL and b"binned tracer" in err()
    assert arr(nb=33, e=None) == M.EINVAL and b"nb 33" in err()
    assert arr(e=None, c=None, s=None) == M.EINVAL and b"null edges" in err()
    assert arr(e=E(e_desc), c=None, s=None) == M.EINVAL and b"edges[2]" in err()
    assert arr(c=None, s=None, ntr=4) == M.EINVAL and b"cnt and bsum" in err()
    assert arr(ntr=4) == M.EINVAL and b"tracer range" in err()
    assert arr(first=1, ntr=3) == M.EINVAL and arr(first=-1) == M.EINVAL and arr(ntr=0) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    # ... and the plan still works; without bsum the tracer range is not looked at
    assert raw(s=None, first=9, ntr=-4) == 0
    p.sync()
    assert_bitwise(to_host(cnt), LH.level_hist(inp["f"], 0, e_h, NB, 0, 0)[0], "the call behind the refused ones")
    assert torch.isnan(bsum).all()
    p.close()


# ---- 7. a multi-GPU handle is refused; the single-device plans of its shards take the call
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
    e_h = LH.call_edges(4, 0)
    cnt = torch.full((4, nz - 1, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    with pytest.raises(M.MpdataError) as e:
        p.level_hist(0, e_h, cnt)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.level_hist_host(0, e_h, np.zeros((ncrms, nz - 1, 4), dt, order="F"))
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.level_hist(9, e_h, cnt)                            # (the handle comes before tc)
    assert e.value.code == M.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all()
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        for j, nb in enumerate((5, 17, 32)):
            triple = TRIPLES[(g + j) % 4]
            Fs = np.asfortranarray(m.a["f"][s0:s0 + nloc])
            edges = LH.call_edges(nb, g + j)
            got = level_hist(M, q, name, triple, edges, nb, OUTS[j], 0, nloc, call=q.level_hist)
            check(got, Fs, triple, edges, nb, f"shard {g} triple {triple} nb {nb}")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 8. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (t1, tn)
FORTRAN = {
    "f64": (F64, "level_hist_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "level_hist_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f32-odd-ref": (F32, "level_hist_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "level_hist_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "level_hist_calls_sp", (4, 2, 72), (1, 2), (1, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: t1 in the 5 bins of edges_a on the block, cnt and bsum of all tracers; tn in the 17 bins of edges_b
    on the whole plan, cnt alone with a tracer range that is not looked at; t1 in the 2 bins of edges_c on the whole plan,
    bsum of tracer tn alone; a call with 33 bins, refused"""
    dt, exe, shape, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = LH.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    ea, eb, ec = LH.call_edges(5, 0), LH.call_edges(17, 4), LH.call_edges(2, 8)
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("edges_a", ea.astype(dt)), ("edges_b", eb.astype(dt)), ("edges_c", ec.astype(dt))]
    # the replay on the model
    m = LH.PlanModelLevelHist(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    cnt_a, bsum_a = m.level_hist(t1, ea, 5, 0, T, sl0=sl0, n=n)
    rc("hist_block"); rc("sync")
    want += [("cnt_a", cnt_a), ("bsum_a", bsum_a)]
    cnt_b, none = m.level_hist(tn, eb, 17, T, 0, bsum=False)
    assert none is None
    rc("hist_cnt"); rc("sync")
    want += [("cnt_b", cnt_b)]
    none, bsum_c = m.level_hist(t1, ec, 2, tn, 1, cnt=False)
    assert none is None
    rc("hist_sum"); rc("sync")
    want += [("bsum_c", bsum_c[..., 0])]
    rc("hist_refused", m.level_hist(t1, eb, 33, 0, 0, bsum=False))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
