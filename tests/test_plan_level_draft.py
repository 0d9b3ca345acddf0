"""GPU tests of the per-level updraft / downdraft sampling of a resident plan (include/mpdata_hip.h 3ac):
mpdata_plan_level_draft_device, the host forms, the array forms, their Python face Plan.level_draft / level_draft_host /
level_draft, and the Fortran program tests/fortran/level_draft_calls.F90.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_draft_model.py: LD.level_draft
on the field and the w the plan holds -- the plan model's (LD.PlanModelLevelDraft: an EXACT plan's f is bit-identical to it;
w is what was uploaded or imported last) or, for FAST plans, the plan's own whole export in front of the call.  The
outputs are filled with NaN and lie between two patterned bands of 4 KiB, which must come back unchanged.  Behind every call
the whole export of f and flux must equal the export taken in front of it, and a run behind the calls must equal the
model's run: the call changed nothing, w included.  On one kind per family the outputs are also held against the existing
Plan.level_cond and Plan.level_stats on the same plan: oracles that do not pass through the new model.

The inputs (LD.make_plan_inputs): every fourth w value is a multiple of 1/8 and two columns of every row are planted with
wc == 0.25 and wc == -0.25, the default thresholds, so the ties occur in most rows; w(:, :, nz) holds nonzero values up to 2,
so a read of it shows.  tests/test_level_draft_cpu.py asserts on the model, for every shape and threshold pair below, that
the seeded variants each change at least one output row in ten.

Plans have three tracers; the (tc; first, ntr) triples are those of 3ab -- (0; 0, 3), (2; 0, 2), (1; 1, 1), (1; 2, 1) -- and
(-1; 0, 3), (-1; 1, 2) without a tracer condition.  With tc >= 0 the bounds rotate through lo and hi, lo alone, hi alone
(LC.call_args: ties c == lo and c == hi in every row, empty rows, full rows) and neither.  The output sets OUTS and the
threshold pairs LD.THRESHOLDS -- on the grid, one-sided infinite, both infinite, wdn == wup -- rotate with other periods.

The kernel has ONE form and no limit in nx of its own; a walk carries 4, 2 or 1 value tracers, so the range lengths 1, 2
and 3 (= 2 + 1) of the triples meet the group sizes, and test_tracer_groups runs plans of 4, 5, 7 and 9 tracers (4, 4 + 1,
4 + 2 + 1, 4 + 4 + 1).  Shapes (ncrms, nx, nz): those of tests/test_plan_level_hist.py (KINDS), the smallest at which a path
of the walk differs (8 columns in flight, 4 in a walk of four tracers)."""
import numpy as np
import pytest

import fortran_records as FR
import level_cond_model as LC
import level_draft_model as LD
import level_stats_model as LS
import plan_harness as H
from oracle import plan_model as PM
from plan_harness import BAND, nan_banded, nan_out, upload
from test_plan_level_hist import BLOCKS, CROSS, FAST, KINDS, PERIODIC, REF, SEED, T
from util import assert_bitwise, bits, to_dev, to_host

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32

TRIPLES = ((0, 0, 3), (2, 0, 2), (1, 1, 1), (1, 2, 1), (-1, 0, 3), (-1, 1, 2))      # (tc, first, ntr)
NAMES4 = ("cnt", "wsum", "fsum", "wfsum")
OUTS = (NAMES4, ("cnt", "wsum"), ("fsum",), ("fsum", "wfsum"), ("wfsum",), ("cnt",), ("wsum", "fsum"), ("cnt", "wfsum"))
BOUNDS = ("both", "lo", "hi", None)
THR = LD.THRESHOLDS

_INPUTS = {}


def inputs(oracle, name):
    """the seven arrays of KINDS[name]: computed once and shared; no test writes them"""
    if name not in _INPUTS:
        shape, ntr, dt, _ = KINDS[name]
        _INPUTS[name] = LD.make_plan_inputs(oracle, shape, ntr, dt, SEED)
    return _INPUTS[name]


def new_plan(M, name, variant=None):
    return H.new_plan(M, KINDS[name], name, name in REF, bool(KINDS[name][3].get("tall")), variant)


def model_of(oracle, name):
    shape, ntr, dt, _ = KINDS[name]
    m = LD.PlanModelLevelDraft(oracle, *shape, ntr, dt)
    assert m.upload({k: np.array(v, order="F") for k, v in inputs(oracle, name).items()}) is None
    return m


def whole(M, p, name, what=("f", "flux")):
    return H.whole(M, p, KINDS[name], what)


def snap(m):
    return {k: np.array(v, order="F") for k, v in m.export_device().items()}


def same(got, want, what):
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def bounds_of(F, tc, kind, seed):
    """(lo, hi) host arrays (n, nzm) or None for the block whose field is F"""
    if tc < 0 or kind is None:
        return None, None
    return LC.call_args(F, tc, kind, seed)


def level_draft(M, p, name, triple, lo, hi, thr, outs, sl0=0, n=None, call=None):
    """Plan.level_draft on block [sl0, sl0 + n) with the outputs `outs` -> {name: host array (n, nzm, 3[, ntr])}.  lo, hi:
    host arrays or None; they lie between NaN bands and must come back unchanged.  The bands are checked.  call: another
    callable with Plan.level_draft's arguments."""
    import torch
    shape, _, dt, _ = KINDS[name]
    nx, nz = shape[1], shape[2]
    n = shape[0] - sl0 if n is None else n
    tc, first, ntr = triple
    sh = M.level_draft_shapes(n, nx, nz, ntr)
    bufs = {key: nan_out(sh[key], dt) for key in NAMES4 if key in outs}
    out = lambda key: bufs[key][2] if key in bufs else None
    ins = {key: nan_banded(a, sh[key]) for key, a in (("lo", lo), ("hi", hi)) if a is not None}
    keep = {key: raw.clone() for key, (raw, _) in ins.items()}
    arg = lambda key: ins[key][1] if key in ins else None
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    (call or p.level_draft)(tc, arg("lo"), arg("hi"), thr[0], thr[1], out("cnt"), out("wsum"), out("fsum"), out("wfsum"), first, sl0, n)
    p.sync()
    torch.cuda.synchronize()
    for key, (raw, _) in ins.items():
        assert torch.equal(raw.view(torch.uint8), keep[key].view(torch.uint8)), f"{key}: an input byte changed"
    res = {}
    for key, (r, pristine, v) in bufs.items():
        assert torch.equal(r[:BAND], pristine[:BAND]) and torch.equal(r[-BAND:], pristine[-BAND:]), f"{key}: a band byte changed"
        res[key] = to_host(v)
    return res


def check(got, F, W, triple, lo, hi, thr, what, sl0=0, n=None):
    """the outputs of level_draft() against the model on block [sl0, sl0 + n) of the fields F and W (lo, hi: the block's)"""
    tc, first, ntr = triple
    n = F.shape[0] - sl0 if n is None else n
    want = dict(zip(NAMES4, LD.level_draft(np.asfortranarray(F[sl0:sl0 + n]), np.asfortranarray(W[sl0:sl0 + n]), tc, lo, hi, thr[0],
                                           thr[1], first, ntr)))
    assert got
    for key, a in got.items():
        assert_bitwise(a, want[key], f"{what}: {key}")


def call_of(k):
    """the rotating arguments of call number k: (triple, bounds kind, thresholds, outputs)"""
    return TRIPLES[k % 6], BOUNDS[(k + k // 6) % 4], THR[(k + k // 4) % len(THR)], OUTS[(k + k // 3) % len(OUTS)]


# ---- 1. every kind of plan: whole plan; triples, bounds, thresholds and output sets rotating; behind the upload (ties on
# the grid) and behind a run (a windowed plan's seams and a periodic plan's halos are stale); a run behind the calls
@pytest.mark.parametrize("name", list(KINDS))
def test_every_plan_kind(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    F0, W0 = inp["f"], inp["w"]
    assert F0.shape == (ncrms, nx + 6, nz - 1, T) and W0.shape == (ncrms, nx + 4, nz) and (W0[:, :, -1] != 0).all()
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
        for j in range(12 if state == "upload" else 7):
            k += 1
            triple, bk, thr, outs = call_of(k + 5 * (state == "run"))
            lo, hi = bounds_of(F, triple[0], bk, 300 + k)
            got = level_draft(M, p, name, triple, lo, hi, thr, outs)
            check(got, F, m.a["w"], triple, lo, hi, thr, f"{name} {state} triple {triple} bounds {bk} thresholds {thr} outputs {outs}")
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
            for j in range(6):
                triple, bk, thr, outs = call_of(40 + 7 * j + (state == "run"))
                lo, hi = bounds_of(before["f"], triple[0], bk, 400 + j)
                got = level_draft(M, p, name, triple, lo, hi, thr, outs)
                check(got, before["f"], W0, triple, lo, hi, thr, f"{name} FAST {state} triple {triple} thresholds {thr}")
            same(whole(M, p, name), before, f"{name} FAST {state}: behind the calls")
        p.close()


# ---- 2. more value tracers than a walk carries: the groups of 4, 2 and 1
@pytest.mark.parametrize("name,TT", [("f64-nz28-nx11", 9), ("f32-nz28-odd", 7), ("f64-nz12-ref", 5), ("f32-nz239-tall-odd", 4),
                                     ("f64-nz28-nx17", 5)])
def test_tracer_groups(mpdata, oracle, name, TT):
    M = mpdata
    shape, _, dt, sw = KINDS[name]
    kind = (shape, TT, dt, sw)
    inp = LD.make_plan_inputs(oracle, shape, TT, dt, SEED + 1)
    p = H.new_plan(M, kind, name, name in REF, bool(sw.get("tall")))
    upload(p, inp)
    for k, (tc, first, ntr, outs) in enumerate(((1, 0, TT, NAMES4), (TT - 1, 1, TT - 1, ("fsum",)), (-1, 0, TT, ("fsum", "wfsum")),
                                                (0, TT - 4, 4, ("wfsum",)), (2, 0, min(TT, 6), ("cnt", "fsum", "wfsum")))):
        thr = THR[k % len(THR)]
        lo, hi = bounds_of(inp["f"], tc, BOUNDS[k % 4], 700 + k)
        import torch
        n, (nx, nz) = shape[0], shape[1:]
        sh = M.level_draft_shapes(n, nx, nz, ntr)
        bufs = {key: nan_out(sh[key], dt) for key in outs}
        out = lambda key: bufs[key][2] if key in bufs else None
        torch.cuda.synchronize()
        p.level_draft(tc, None if lo is None else to_dev(lo), None if hi is None else to_dev(hi), thr[0], thr[1], out("cnt"), out("wsum"),
                      out("fsum"), out("wfsum"), first)
        p.sync()
        torch.cuda.synchronize()
        got = {}
        for key, (r, pristine, v) in bufs.items():
            assert H.bands_kept(r, pristine), key
            got[key] = to_host(v)
        check(got, inp["f"], inp["w"], (tc, first, ntr), lo, hi, thr, f"{name} with {TT} tracers: tc {tc} range {first, ntr} outputs {outs}")
    p.close()


# ---- 3. the existing calls on the same plan: with wup = +inf, wdn = -inf the ENV class has the bits of level_cond's cnt and
# csum (tc = -1: of level_stats' sum, and cnt = nx), UP and DOWN are +0; with any thresholds the three counts add up to
# level_cond's cnt
@pytest.mark.parametrize("name", CROSS)
def test_classes_against_level_cond_and_level_stats(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    tdt = H.tdt(dt)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    inf = float("inf")
    pos0 = lambda a: not a.any() and not np.signbit(a).any()
    for state in ("upload", "run"):
        if state == "run":
            p.run()
        F = whole(M, p, name, ("f",))["f"]
        for j, (tc, first, ntr_) in enumerate(TRIPLES[:4]):
            bk = BOUNDS[j % 3]
            lo, hi = bounds_of(F, tc, bk, 450 + j)
            sh = M.level_cond_shapes(ncrms, nx, nz, ntr_)
            c1 = torch.full(sh["cnt"], float("nan"), dtype=tdt, device="cuda:0")
            s1 = torch.full(sh["csum"], float("nan"), dtype=tdt, device="cuda:0")
            torch.cuda.synchronize()
            p.level_cond(tc, None if lo is None else to_dev(lo), None if hi is None else to_dev(hi), c1, s1, first)
            p.sync()
            got = level_draft(M, p, name, (tc, first, ntr_), lo, hi, (inf, -inf), NAMES4)
            what = f"{name} {state} triple {tc, first, ntr_} bounds {bk}"
            assert_bitwise(got["cnt"][:, :, LD.ENV], to_host(c1), what + ": cnt(ENV) against level_cond")
            assert_bitwise(got["fsum"][:, :, LD.ENV, :], to_host(s1), what + ": fsum(ENV) against level_cond")
            for key in NAMES4:
                assert pos0(got[key][:, :, LD.UP]) and pos0(got[key][:, :, LD.DOWN]), (what, key)
            for thr in THR[:3] + THR[4:]:
                cnt = level_draft(M, p, name, (tc, first, ntr_), lo, hi, thr, ("cnt",))["cnt"]
                assert_bitwise(np.asfortranarray(cnt.sum(axis=2)), to_host(c1), what + f" thresholds {thr}: the counts add up")
        # no tracer condition: level_stats
        sm = torch.full((T, nz - 1, ncrms), float("nan"), dtype=tdt, device="cuda:0")
        torch.cuda.synchronize()
        p.level_stats(sum=sm)
        p.sync()
        got = level_draft(M, p, name, (-1, 0, T), None, None, (inf, -inf), ("cnt", "fsum"))
        assert_bitwise(got["fsum"][:, :, LD.ENV, :], to_host(sm), f"{name} {state}: fsum(ENV) against level_stats")
        assert (got["cnt"][:, :, LD.ENV] == nx).all() and pos0(got["cnt"][:, :, :2]) and pos0(got["fsum"][:, :, :2])
    p.close()


# ---- 4. blocks: only the block's instances reach the outputs, and nothing else is written
@pytest.mark.parametrize("name", list(BLOCKS))
def test_blocks_reach_only_their_outputs(mpdata, oracle, name):
    """the arguments rotate over the blocks, each block with three calls; a run between the blocks"""
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
            triple, bk, thr, outs = call_of(7 * b + 3 * j + 1)
            F = m.a["f"]
            lo, hi = bounds_of(np.asfortranarray(F[sl0:sl0 + n]), triple[0], bk, 500 + 10 * b + j)
            got = level_draft(M, p, name, triple, lo, hi, thr, outs, sl0, n)
            check(got, F, m.a["w"], triple, lo, hi, thr, f"{name} block {sl0, n} triple {triple} thresholds {thr} outputs {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} block {sl0, n}: behind the calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name}: a run behind the calls")
    p.close()


# ---- 5. selection means selection: +inf and NaN in every cell of a value tracer OUTSIDE a class never reach that class
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz239-tall"])
def test_cells_outside_a_class_reach_no_sum_of_it(mpdata, oracle, name):
    M = mpdata
    inp = inputs(oracle, name)
    F0, W0 = inp["f"], inp["w"]
    p = new_plan(M, name)
    upload(p, inp)
    for k, (tc, t, cls) in enumerate(((0, 2, LD.ENV), (2, 1, LD.UP), (1, 0, LD.DOWN), (-1, 1, LD.ENV))):
        thr = (LD.WUP, LD.WDN)
        lo, hi = bounds_of(F0, tc, "both", 800 + k)
        P = LD.plant(F0, W0, tc, lo, hi, thr[0], thr[1], t, cls)
        assert np.isnan(P[..., t]).any() and np.isposinf(P[..., t]).any()
        want = LD.level_draft(P, W0, tc, lo, hi, thr[0], thr[1], 0, T)
        assert np.isfinite(want[2][:, :, cls]).all() and np.isfinite(want[3][:, :, cls]).all()
        bad = LD.level_draft(P, W0, tc, lo, hi, thr[0], thr[1], t, 1, multiply=True)
        assert not np.isfinite(bad[2][:, :, cls]).all() and not np.isfinite(bad[3][:, :, cls]).all()
        p.import_device(f=to_dev(np.asfortranarray(P[..., t])), first_tracer=t)
        for triple in ((tc, 0, T), (tc, t, 1)):
            got = level_draft(M, p, name, triple, lo, hi, thr, NAMES4)
            w = LD.level_draft(P, W0, tc, lo, hi, thr[0], thr[1], triple[1], triple[2])
            for key, a in zip(NAMES4, w):
                assert np.isfinite(got[key][:, :, cls]).all(), (name, triple, key)
                # (the other classes hold NaNs whose payloads are not defined: their finite cells and their NaN cells must agree)
                assert_bitwise(np.asfortranarray(got[key][:, :, cls]), np.asfortranarray(a[:, :, cls]),
                               f"{name} planted tracer {t} outside class {cls} under tc {tc} triple {triple}: {key}")
                fin = np.isfinite(a)
                assert np.array_equal(np.isnan(got[key]), np.isnan(a)) and np.array_equal(bits(got[key])[fin], bits(a)[fin]), (name, key)
        p.import_device(f=to_dev(np.asfortranarray(F0[..., t])), first_tracer=t)
    p.close()


# ---- 6. the host form and the array forms
@pytest.mark.parametrize("name", ["f64-nz28-nx11", "f32-nz28-odd", "f64-nz12-ref", "f64-nz72", "f64-nz239-tall"])
def test_host_form(mpdata, oracle, name):
    M = mpdata
    shape, ntr, dt, sw = KINDS[name]
    ncrms, nx, nz = shape
    # (sl0, n, tc, bounds, thresholds, outputs): all tracers
    script = ((0, ncrms, 0, "both", THR[0], NAMES4), (1, ncrms - 1, 2, "lo", THR[1], ("fsum",)), (ncrms - 1, 1, -1, None, THR[0], ("cnt", "wsum")),
              (0, 2, 1, "hi", THR[4], ("wfsum",)), (0, ncrms, -1, None, THR[3], ("cnt", "fsum", "wfsum")))
    m = model_of(oracle, name)
    p = new_plan(M, name)
    upload(p, inputs(oracle, name))
    p.run()
    assert m.run() is None
    before = whole(M, p, name)
    for k, (sl0, n, tc, bk, thr, outs) in enumerate(script):
        lo, hi = bounds_of(np.asfortranarray(m.a["f"][sl0:sl0 + n]), tc, bk, 600 + k)
        new = lambda key, *tail: np.full((n, nz - 1, 3) + tail, np.nan, dt, order="F") if key in outs else None
        a = {"cnt": new("cnt"), "wsum": new("wsum"), "fsum": new("fsum", T), "wfsum": new("wfsum", T)}
        keep = [None if x is None else np.array(x) for x in (lo, hi)]
        p.level_draft_host(tc, lo, hi, thr[0], thr[1], a["cnt"], a["wsum"], a["fsum"], a["wfsum"], sl0, n)
        for x, y in zip((lo, hi), keep):
            assert x is None or np.array_equal(bits(x), bits(y))
        check({key: v for key, v in a.items() if v is not None}, m.a["f"], m.a["w"], (tc, 0, T), lo, hi, thr,
              f"{name} host form {sl0, n} tc {tc} {outs}", sl0, n)
        same(whole(M, p, name), before, f"{name} host form {sl0, n}")
    with pytest.raises(M.MpdataError):
        p.level_draft_host(-1, None, None, 0.0, 0.0, np.zeros((ncrms, nz - 2, 3), dt, order="F"))      # a wrong shape
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), f"{name} host form: a run behind the calls")
    p.close()


# 257 and 600 instances: more than one block of 256 threads and a partly filled last one; (2, 3, 70000): the second trip over
# gridDim.y.  Each with a block inside the arrays (sl0 > 0).  The last call plants +inf and NaN outside the ENV class.
ARRAYS = {"n257": ((257, 3, 6), 3, (1, 256)), "n600": ((600, 2, 5), 4, (300, 299)), "rows70000": ((2, 3, 70000), 3, (1, 1)),
          "nx17": ((5, 17, 4), 3, (2, 2))}


@pytest.mark.parametrize("case", list(ARRAYS))
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_array_forms(mpdata, dt, case):
    import torch
    M = mpdata
    (ncrms, nx, nz), ntr_all, (b0, bn) = ARRAYS[case]
    rng = np.random.default_rng([78, ncrms, ntr_all])
    f = np.asfortranarray(rng.uniform(-1, 2, (ncrms, nx + 6, nz - 1, ntr_all)).astype(dt))
    w = rng.uniform(-0.5, 0.5, (ncrms, nx + 4, nz))
    w = np.asfortranarray(np.where(rng.integers(0, 2, w.shape) == 0, np.round(w * 8) / 8, w).astype(dt))
    w[:, :, -1] = dt(3)
    # ((sl0, n), (tc, first, ntr), bounds, thresholds, outputs, planted tracer or None, with f)
    calls = (((0, ncrms), (0, 0, ntr_all), "both", THR[0], NAMES4, None, True), ((b0, bn), (ntr_all - 1, 0, 2), "lo", THR[1], ("fsum",), None, True),
             ((b0, bn), (-1, 0, 0), None, THR[0], ("cnt", "wsum"), None, False), ((0, ncrms), (1, 0, 1), "hi", THR[4], ("wfsum",), None, True),
             ((b0, bn), (-1, 1, 2), None, THR[3], ("cnt", "fsum", "wfsum"), None, True), ((b0, bn), (1, 2, 1), "both", THR[0], NAMES4, 2, True))
    if case == "rows70000":
        calls = calls[1:3] + calls[5:]
    wd = to_dev(w)
    for k, ((sl0, n), (tc, first, ntr), bk, thr, outs, planted, with_f) in enumerate(calls):
        fb, wb = np.asfortranarray(f[sl0:sl0 + n]), np.asfortranarray(w[sl0:sl0 + n])
        lo, hi = bounds_of(fb, tc, bk, 900 + k)
        g = f
        if planted is not None:
            g = np.array(f, order="F")
            g[sl0:sl0 + n] = LD.plant(fb, wb, tc, lo, hi, thr[0], thr[1], planted, LD.ENV)
            assert not np.isfinite(g[..., planted]).all()
        fd = to_dev(g) if with_f else None
        want = dict(zip(NAMES4, LD.level_draft(np.asfortranarray(g[sl0:sl0 + n]) if with_f else None, wb, tc, lo, hi, thr[0], thr[1],
                                               first, ntr)))
        sh = M.level_draft_shapes(n, nx, nz, ntr)
        bufs = {key: nan_out(sh[key], dt) for key in outs}
        out = lambda key: bufs[key][2] if key in bufs else None
        torch.cuda.synchronize()
        M.level_draft(fd, wd, tc, None if lo is None else to_dev(lo), None if hi is None else to_dev(hi), thr[0], thr[1], out("cnt"),
                      out("wsum"), out("fsum"), out("wfsum"), first, sl0, n)
        torch.cuda.synchronize()
        for key, (r, pristine, v) in bufs.items():
            assert H.bands_kept(r, pristine), key
            a, b = to_host(v), want[key]
            what = f"array form {case} block {sl0, n} triple {tc, first, ntr} thresholds {thr}: {key}"
            if planted is None:
                assert_bitwise(a, b, what)
            else:
                assert np.isfinite(a[:, :, LD.ENV]).all()
                assert_bitwise(np.asfortranarray(a[:, :, LD.ENV]), np.asfortranarray(b[:, :, LD.ENV]), what)
        if with_f:
            assert_bitwise(to_host(fd), g, f"array form {case}: f is only read")
    assert_bitwise(to_host(wd), w, f"array form {case}: w is only read")


# ---- 7. every error code, in the stated order; the plan's state before and after; every refusal leaves the outputs NaN;
# behind run_uw the plan does not hold w until w has been imported whole again -- w alone, u is not needed
def test_errors_change_nothing(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-nz28-nx11"
    shape, ntr, dt, _ = KINDS[name]
    ncrms, nx, nz = shape
    inp = inputs(oracle, name)
    nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device="cuda:0")
    cnt, wsum, fsum, wfsum = nan(3, nz - 1, ncrms), nan(3, nz - 1, ncrms), nan(T, 3, nz - 1, ncrms), nan(T, 3, nz - 1, ncrms)
    lo = torch.zeros((nz - 1, ncrms), dtype=torch.float64, device="cuda:0")
    qnan, inf = float("nan"), float("inf")

    def code(fn, *a, **kw):
        with pytest.raises(M.MpdataError) as e:
            fn(*a, **kw)
        return e.value.code

    p = new_plan(M, name)
    assert code(p.level_draft, 0, lo, None, 0.25, -0.25, cnt) == M.ESTATE                    # never filled
    assert code(p.level_draft, 3, lo, None, 0.25, -0.25, cnt) == M.EINVAL                    # ... the arguments come first
    upload(p, inp)
    m = model_of(oracle, name)
    before = whole(M, p, name)
    L = M.lib()
    err = L.mpdata_last_error
    P = lambda t: None if t is None else t.data_ptr()
    raw = lambda sl0=0, n=ncrms, tc=0, lo=lo, hi=None, wup=0.25, wdn=-0.25, c=cnt, ws=wsum, fs=fsum, wf=wfsum, first=0, ntr=T: \
        L.mpdata_plan_level_draft_device(p._p, sl0, n, tc, P(lo), P(hi), wup, wdn, P(c), P(ws), P(fs), P(wf), first, ntr)
    assert raw(ws=None, fs=None, wf=None, ntr=0) == 0                                        # (the lambda itself is right)
    p.sync()
    cnt.fill_(qnan)
    assert L.mpdata_plan_level_draft_device(None, 0, ncrms, 0, P(lo), None, 0.25, -0.25, P(cnt), None, None, None, 0, T) == M.EINVAL
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (3, 3)):
        assert raw(sl0, n) == M.EINVAL, (sl0, n)
    for tc in (-2, 3, 9):
        assert raw(tc=tc) == M.EINVAL and b"condition tracer" in err(), tc
    assert raw(tc=-1) == M.EINVAL and b"without a condition tracer" in err()
    assert raw(tc=-1, lo=None, hi=lo) == M.EINVAL and b"without a condition tracer" in err()
    assert raw(wup=qnan) == M.EINVAL and b"NaN" in err() and raw(wdn=qnan) == M.EINVAL and b"NaN" in err()
    assert raw(wup=-0.25, wdn=0.25) == M.EINVAL and b"wdn" in err() and raw(wup=-inf, wdn=inf) == M.EINVAL
    assert raw(c=None, ws=None, fs=None, wf=None) == M.EINVAL and b"all NULL" in err()
    for first, n_ in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert raw(first=first, ntr=n_) == M.EINVAL and b"tracer range" in err(), (first, n_)
        assert raw(first=first, ntr=n_, c=None, ws=None, fs=None) == M.EINVAL and b"tracer range" in err()      # wfsum alone asks too
    # the order: the range, tc, lo / hi without tc, the thresholds, the outputs, the tracers
    assert raw(0, 0, 9, wup=qnan, c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"n = 0" in err()
    assert raw(tc=9, wup=qnan, c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"condition tracer" in err()
    assert raw(tc=-1, wup=qnan, c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"without a condition" in err()
    assert raw(wup=qnan, c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"NaN" in err()
    assert raw(wup=0.0, wdn=1.0, c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"wdn" in err()
    assert raw(c=None, ws=None, fs=None, wf=None, first=9) == M.EINVAL and b"all NULL" in err()
    assert raw(first=9) == M.EINVAL and b"tracer range" in err()
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (cnt, wsum, fsum, wfsum))                        # no refused call wrote an output
    # a host form of the other precision; its arguments come first
    c32 = np.full((ncrms, nz - 1, 3), np.nan, F32, order="F")
    h32 = lambda tc=-1, wup=0.25, c=c32.ctypes.data: L.mpdata_plan_level_draft_f32(p._p, 0, ncrms, tc, None, None, wup, -0.25, c, None, None, None)
    assert h32() == M.ESTATE
    assert h32(c=None) == M.EINVAL and b"all NULL" in err()
    assert h32(tc=3) == M.EINVAL and h32(wup=qnan) == M.EINVAL
    assert np.isnan(c32).all()
    # the array forms: sizes, the block, w, f where it is needed, then tc, the bounds, the thresholds, the outputs, the tracers
    arr = lambda ncrms=4, nz=6, sl0=0, n=4, f=8, w=8, tc=0, lo=8, wup=0.25, wdn=-0.25, c=8, fs=8, first=0, ntr=3: \
        L.mpdata_level_draft_device(ncrms, 5, nz, 3, sl0, n, f, w, tc, lo, None, wup, wdn, c, None, fs, None, first, ntr, None)
    assert arr(nz=1, sl0=2, n=3, w=None, tc=3) == M.EINVAL and b"nz=1" in err()
    assert arr(sl0=2, n=3, w=None, tc=3) == M.EINVAL and b"outside" in err()
    assert arr(w=None, f=None, tc=3) == M.EINVAL and b"null w" in err()
    assert arr(f=None, tc=3) == M.EINVAL and b"null f" in err()
    assert arr(f=None, tc=-1, lo=None) == M.EINVAL and b"null f" in err()                     # fsum reads f
    assert arr(f=None, tc=0, fs=None) == M.EINVAL and b"null f" in err()                      # the condition reads f
    assert arr(tc=3, wup=qnan) == M.EINVAL and b"condition tracer" in err()
    assert arr(tc=-1, wup=qnan) == M.EINVAL and b"without a condition" in err()
    assert arr(wup=qnan, c=None, fs=None) == M.EINVAL and b"NaN" in err()
    assert arr(wup=-1.0, wdn=1.0, c=None, fs=None) == M.EINVAL and b"wdn" in err()
    assert arr(c=None, fs=None, ntr=4) == M.EINVAL and b"all NULL" in err()
    assert arr(ntr=4) == M.EINVAL and b"tracer range" in err()
    assert arr(first=1, ntr=3) == M.EINVAL and arr(first=-1) == M.EINVAL and arr(ntr=0) == M.EINVAL
    after = whole(M, p, name)
    for k in before:
        assert_bitwise(after[k], before[k], f"after the refused calls: {k}")
    # ... and the plan still works; without fsum and wfsum the tracer range is not looked at
    assert raw(lo=None, ws=None, fs=None, wf=None, first=9, ntr=-4) == 0
    p.sync()
    assert_bitwise(to_host(cnt), LD.level_draft(inp["f"], inp["w"], 0, None, None, 0.25, -0.25, 0, 0)[0], "the call behind the refused ones")
    assert all(torch.isnan(t).all() for t in (wsum, fsum, wfsum))
    # run_uw uses the plan's velocities up: MPDATA_ESTATE until w has been imported whole again; u is not needed
    other = oracle.make_inputs(*shape, seed=SEED + 50, dist=oracle.DIST_RAW_SIGNED, dtype=dt)
    ou, ow = other["u"], other["w"]
    p.run_uw(to_dev(ou), to_dev(ow))
    assert m.run_uw(ou, ow) is None
    cnt.fill_(qnan)
    assert raw(lo=None, ws=None, fs=None, wf=None) == M.ESTATE and b"does not hold w" in err()
    assert raw(tc=9) == M.EINVAL                                                             # (the arguments still come first)
    assert m.level_draft(0) == PM.ESTATE
    p.import_device(u=to_dev(ou))
    assert m.import_device({"u": ou}) is None
    assert raw(lo=None, ws=None, fs=None, wf=None) == M.ESTATE and m.level_draft(0) == PM.ESTATE       # u alone does not help
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all()
    p.close()
    # a plan that holds w but not u
    p = new_plan(M, name)
    upload(p, inp)
    m = model_of(oracle, name)
    p.run_uw(to_dev(ou), to_dev(ow))
    assert m.run_uw(ou, ow) is None
    w2 = LD.make_plan_inputs(oracle, shape, T, dt, SEED + 9)["w"]
    p.import_device(w=to_dev(w2))
    assert m.import_device({"w": w2}) is None and m.have_w and not m.have_u
    for k in range(4):
        triple, bk, thr, outs = call_of(11 + 5 * k)
        lo_h, hi_h = bounds_of(m.a["f"], triple[0], bk, 950 + k)
        got = level_draft(M, p, name, triple, lo_h, hi_h, thr, outs)
        check(got, m.a["f"], w2, triple, lo_h, hi_h, thr, f"behind run_uw and an import of w alone: triple {triple} thresholds {thr}")
    assert code(p.run) == M.ESTATE                                                           # (u is still missing: the call lent nothing)
    p.import_device(u=to_dev(ou))
    assert m.import_device({"u": ou}) is None
    p.run()
    assert m.run() is None
    same(whole(M, p, name), snap(m), "behind run_uw, the imports, the calls and a run")
    p.close()


# ---- 8. a multi-GPU handle is refused; the single-device plans of its shards take the call
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
    cnt = torch.full((3, nz - 1, ncrms), float("nan"), dtype=torch.float64, device="cuda:0")
    with pytest.raises(M.MpdataError) as e:
        p.level_draft(-1, None, None, 0.25, -0.25, cnt)
    assert e.value.code == M.EUNSUPPORTED and b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    with pytest.raises(M.MpdataError) as e:
        p.level_draft_host(-1, None, None, 0.25, -0.25, np.zeros((ncrms, nz - 1, 3), dt, order="F"))
    assert e.value.code == M.EUNSUPPORTED
    with pytest.raises(M.MpdataError) as e:
        p.level_draft(9, None, None, float("nan"), -0.25, cnt)                 # (the handle comes before tc and the thresholds)
    assert e.value.code == M.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all()
    same(whole(M, p, name), m.export_device(), "after the refused handle calls")
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        for j in range(3):
            triple, bk, thr, outs = call_of(3 * g + j + 2)
            Fs, Ws = np.asfortranarray(m.a["f"][s0:s0 + nloc]), np.asfortranarray(m.a["w"][s0:s0 + nloc])
            lo, hi = bounds_of(Fs, triple[0], bk, 970 + j)
            got = level_draft(M, q, name, triple, lo, hi, thr, outs, 0, nloc, call=q.level_draft)
            check(got, Fs, Ws, triple, lo, hi, thr, f"shard {g} triple {triple} thresholds {thr}")
        q.close()
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls")
    p.run()
    assert m.run() is None
    same(whole(M, p, name), m.export_device(), "after the shard plans' calls and a run")
    p.close()


# ---- 9. the Fortran program: every record of its dump against the model
# dtype, program, shape, block, (t1, tn)
FORTRAN = {
    "f64": (F64, "level_draft_calls", (7, 5, 10), (2, 3), (0, 2)), "f32": (F32, "level_draft_calls_sp", (6, 5, 10), (1, 3), (2, 0)),
    "f32-odd-ref": (F32, "level_draft_calls_sp", (7, 3, 12), (6, 1), (0, 2)),
    "f64-nz72": (F64, "level_draft_calls", (3, 2, 72), (1, 2), (2, 0)), "f32-nz72": (F32, "level_draft_calls_sp", (4, 2, 72), (1, 2), (1, 1)),
}


@pytest.mark.parametrize("case", list(FORTRAN))
def test_fortran_program_matches_the_model(oracle, tmp_path, case):
    """the program's calls: t1 inside (lo_a, hi_a] on the block against (wup, wdn), all four outputs of all tracers; no tracer
    condition on the whole plan, cnt and wsum alone with a tracer range that is not looked at; tn up to hi_c on the whole
    plan against (wup, -inf), wfsum of tracer t1 alone; a call with wdn > wup, refused"""
    dt, exe, shape, (sl0, n), (t1, tn) = FORTRAN[case]
    ncrms, nx, nz = shape
    inp = LD.make_plan_inputs(oracle, shape, T, dt, SEED + 3)
    lo_a, hi_a = LC.call_args(np.asfortranarray(inp["f"][sl0:sl0 + n]), t1, "both", 1)
    _, hi_c = LC.call_args(inp["f"], tn, "hi", 2)
    wup, wdn = LD.WUP, LD.WDN
    records = [("params", np.array([ncrms, nx, nz, T, sl0, n, t1, tn], np.int64))]
    records += [(k, inp[k]) for k in PM.NAMES] + [("thr", np.array([wup, wdn], dt)), ("lo_a", lo_a), ("hi_a", hi_a), ("hi_c", hi_c)]
    # the replay on the model
    m = LD.PlanModelLevelDraft(oracle, ncrms, nx, nz, T, dt)
    want = FR.want_import(m, inp)
    rc = lambda what, code=None: want.append(FR.rc(what, code))
    a = m.level_draft(t1, lo_a, hi_a, wup, wdn, 0, T, sl0=sl0, n=n)
    rc("draft_block"); rc("sync")
    want += [("cnt_a", a[0]), ("wsum_a", a[1]), ("fsum_a", a[2]), ("wfsum_a", a[3])]
    b = m.level_draft(-1, None, None, wup, wdn, T, 0, fsum=False, wfsum=False)
    assert b[2] is None and b[3] is None
    rc("draft_w"); rc("sync")
    want += [("cnt_b", b[0]), ("wsum_b", b[1])]
    c = m.level_draft(tn, None, hi_c, wup, -np.inf, t1, 1, cnt=False, wsum=False, fsum=False)
    assert c[0] is None and c[1] is None and c[2] is None
    rc("draft_up"); rc("sync")
    want += [("wfsum_c", c[3][..., 0])]
    rc("draft_refused", m.level_draft(t1, None, None, wdn, wup, 0, 0, fsum=False, wfsum=False, wsum=False))
    want += FR.want_close(m)
    FR.compare_dump(FR.run_program(exe, records, tmp_path), want, case)
