"""Tests without a GPU of the per-level updraft / downdraft sampling (include/mpdata_hip.h 3ac): the numpy model of
tests/level_draft_model.py against tests/level_cond_model.py and tests/level_stats_model.py (the three bit relations of the
header), the edge rules, the variants the GPU tests must tell apart, the plan model's check order, and the interface -- the
header section, the prototype table of capi.py, the Fortran module, the argument checks that need no device and the
resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import level_cond_model as LC
import level_draft_model as LD
import level_stats_model as LS
from oracle import plan_model as PM
from test_plan_level_draft import BOUNDS, KINDS, SEED, THR, TRIPLES
from test_plan_level_draft_sequences import CASES
from util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_draft_device", "mpdata_plan_level_draft", "mpdata_plan_level_draft_f32", "mpdata_level_draft_device",
         "mpdata_level_draft_f32_device")
DTYPES = [np.float64, np.float32]
SHAPES = sorted({(k[0], np.dtype(k[2]).name) for k in KINDS.values()} | {(c[1], np.dtype(c[3]).name) for c in CASES})
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{d}" for s, d in SHAPES]
INF = float("inf")


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def pos0(a):
    return not a.any() and not np.signbit(a).any()


def fields(n, nx, nz, T, dtype, seed):
    rng = np.random.default_rng(seed)
    f = np.asfortranarray(rng.uniform(-1, 2, (n, nx + 6, nz - 1, T)).astype(dtype))
    w = rng.uniform(-0.5, 0.5, (n, nx + 4, nz))
    w = np.asfortranarray(np.where(rng.integers(0, 2, w.shape) == 0, np.round(w * 8) / 8, w).astype(dtype))
    w[:, :, -1] = 1000
    return f, w


# ---- the three bit relations of the header, against the models of 3v and 3g, on every shape of the GPU tests
@pytest.mark.parametrize("shape,dtn", SHAPES, ids=IDS)
def test_bit_relations_to_level_cond_and_level_stats(oracle, shape, dtn):
    dt = np.dtype(dtn).type
    inp = LD.make_plan_inputs(oracle, shape, 3, dt, SEED)
    F, W = inp["f"], inp["w"]
    n, nx, nzm = shape[0], shape[1], shape[2] - 1
    for j, (tc, first, ntr) in enumerate(TRIPLES[:4]):
        lo, hi = LC.call_args(F, tc, BOUNDS[j % 3], 40 + j)
        q, s = LC.level_cond(F, tc, lo, hi, first, ntr)
        cnt, wsum, fsum, wfsum = LD.level_draft(F, W, tc, lo, hi, INF, -INF, first, ntr)
        assert cnt.shape == wsum.shape == (n, nzm, 3) and fsum.shape == wfsum.shape == (n, nzm, 3, ntr)
        assert all(a.dtype == dt for a in (cnt, wsum, fsum, wfsum))
        assert same(np.asfortranarray(cnt[:, :, LD.ENV]), q) and same(np.asfortranarray(fsum[:, :, LD.ENV]), s)
        for a in (cnt, wsum, fsum, wfsum):
            assert pos0(a[:, :, LD.UP]) and pos0(a[:, :, LD.DOWN])
        for wup, wdn in THR:
            c = LD.level_draft(F, W, tc, lo, hi, wup, wdn, 0, 0)[0]
            assert same(np.asfortranarray(c.sum(axis=2)), q), (wup, wdn)
    cnt, _, fsum, _ = LD.level_draft(F, W, -1, None, None, INF, -INF, 0, 3)
    assert same(np.asfortranarray(fsum[:, :, LD.ENV]), LS.level_stats(F)[0]) and (cnt[:, :, LD.ENV] == nx).all()
    assert pos0(cnt[:, :, :2]) and pos0(fsum[:, :, :2])
    if nzm <= 30:
        lo, hi = LC.call_args(F, 1, "both", 44)
        for x, y in zip(LD.level_draft(F, W, 1, lo, hi), LD.level_draft_loops(F, W, 1, lo, hi)):
            assert same(x, np.asfortranarray(y))


# ---- the edge rules
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rules(dtype):
    dt = np.dtype(dtype).type
    F, W = fields(3, 9, 6, 2, dtype, 5)
    n, nx, nzm = 3, 9, 5
    # wc == wup and wc == wdn are ENV
    G = np.array(W)
    G[:, 2:nx + 2, :] = dt(0.25)                                  # wc = 0.25 below the top, 0.125 at the top level
    cnt = LD.level_draft(None, G, -1, None, None, 0.25, -0.25, 0, 0)[0]
    assert (cnt[:, :, LD.ENV] == nx).all() and pos0(cnt[:, :, :2])
    cnt = LD.level_draft(None, -G, -1, None, None, 0.25, -0.25, 0, 0)[0]
    assert (cnt[:, :, LD.ENV] == nx).all() and pos0(cnt[:, :, :2])
    cnt = LD.level_draft(None, G, -1, None, None, 0.25, -0.25, 0, 0, ge=True)[0]
    assert (cnt[:, :-1, LD.UP] == nx).all() and (cnt[:, -1, LD.ENV] == nx).all()
    # the top level takes +0 for wk1: level nz of w is never read
    H = np.array(G)
    H[:, :, -1] = dt(-77)
    for x, y in zip(LD.level_draft(F, G, 0, None, None, 0.2, 0.1), LD.level_draft(F, H, 0, None, None, 0.2, 0.1)):
        assert same(x, y)
    assert (LD.level_draft(None, G, -1, None, None, 0.2, 0.1, 0, 0)[0][:, -1, LD.ENV] == nx).all()      # 0.125: neither above 0.2 nor below 0.1
    # -0.0 against a threshold of 0: equal, so neither above nor below; the sum of wc is -0.0 + ... from +0: +0
    G[:, 2:nx + 2, :] = dt(-0.0)
    for z in (0.0, -0.0):
        cnt, wsum, _, _ = LD.level_draft(None, G, -1, None, None, z, z, 0, 0)
        assert (cnt[:, :, LD.ENV] == nx).all() and pos0(cnt[:, :, :2]) and pos0(wsum)
    # wdn == wup: ENV holds exactly the ties
    cnt = LD.level_draft(None, W, -1, None, None, 0.125, 0.125, 0, 0)[0]
    wk1 = np.concatenate([W[:, 2:nx + 2, 1:nzm], np.zeros((n, nx, 1), dtype)], axis=2)
    wc = dt(0.5) * (W[:, 2:nx + 2, :nzm] + wk1)
    assert np.array_equal(cnt[:, :, LD.ENV], (wc == dt(0.125)).sum(axis=1)) and (wc == dt(0.125)).any()
    assert np.array_equal(cnt[:, :, LD.UP], (wc > dt(0.125)).sum(axis=1)) and np.array_equal(cnt[:, :, LD.DOWN], (wc < dt(0.125)).sum(axis=1))
    # infinite thresholds: one-sided classes
    cnt = LD.level_draft(None, W, -1, None, None, INF, -0.1, 0, 0)[0]
    assert pos0(cnt[:, :, LD.UP]) and cnt[:, :, LD.DOWN].any() and (cnt.sum(axis=2) == nx).all()
    cnt = LD.level_draft(None, W, -1, None, None, 0.1, -INF, 0, 0)[0]
    assert pos0(cnt[:, :, LD.DOWN]) and cnt[:, :, LD.UP].any() and (cnt.sum(axis=2) == nx).all()
    cnt = LD.level_draft(None, W, -1, None, None, -INF, -INF, 0, 0)[0]
    assert (cnt[:, :, LD.UP] == nx).all()
    # tc = -1: every column is in a class; a column that is not in_i is in none
    lo, hi = LC.call_args(F, 0, "both", 3)
    cnt = LD.level_draft(F, W, 0, lo, hi, 0.1, -0.1, 0, 0)[0]
    assert same(np.asfortranarray(cnt.sum(axis=2)), LC.level_cond(F, 0, lo, hi, 0, 0)[0]) and (cnt.sum(axis=2) < nx).any()
    # wsum and wfsum are sums of wc and of the per-column product
    cnt, wsum, fsum, wfsum = LD.level_draft(F, W, -1, None, None, INF, -INF, 1, 1)
    s = np.zeros((n, nzm), dtype)
    sp = np.zeros((n, nzm), dtype)
    for i in range(nx):
        s = s + wc[:, i]
        sp = sp + wc[:, i] * F[:, 3 + i, :, 1]
    assert same(np.asfortranarray(wsum[:, :, LD.ENV]), np.asfortranarray(s)) and same(np.asfortranarray(wfsum[:, :, LD.ENV, 0]), np.asfortranarray(sp))
    # inf or NaN in a value cell outside a class reaches no sum of the class; a multiplied mask lets it in
    for cls in (LD.UP, LD.DOWN, LD.ENV):
        P = LD.plant(F, W, 0, lo, hi, 0.1, -0.1, 1, cls)
        assert np.isnan(P[..., 1]).any() and np.isposinf(P[..., 1]).any()
        good = LD.level_draft(P, W, 0, lo, hi, 0.1, -0.1, 0, 2)
        assert np.isfinite(good[2][:, :, cls]).all() and np.isfinite(good[3][:, :, cls]).all()
        bad = LD.level_draft(P, W, 0, lo, hi, 0.1, -0.1, 1, 1, multiply=True)
        assert not np.isfinite(bad[2][:, :, cls]).all() and not np.isfinite(bad[3][:, :, cls]).all()
    # the thresholds are rounded once to the fields' precision
    if dtype == np.float32:
        third = 1 / 3
        G[:, 2:nx + 2, :] = np.float32(third)                     # wc = float32(1/3) > 1/3 as a double, == the rounded threshold
        cnt = LD.level_draft(None, G, -1, None, None, third, -1.0, 0, 0)[0]
        assert (cnt[:, :-1, LD.ENV] == nx).all()


# ---- the shapes of the GPU tests: the inputs tell the variants apart
@pytest.mark.parametrize("shape,dtn", SHAPES, ids=IDS)
def test_inputs_tell_the_variants_apart(oracle, shape, dtn):
    """On the fields the GPU tests upload, over their four triples with a condition tracer (bounds rotating; the two without
    one put every column into a class and only raise the shares), for every threshold pair of
    LD.THRESHOLDS each variant changes at least one output row in ten, wherever it is another function at all:
      ge (>= for >, <= for <) and swap (UP and DOWN exchanged) on every pair with a finite threshold -- with wup = +inf and
        wdn = -inf no w of the contract reaches a threshold and both draft classes are empty, so the variants ARE the
        definition there, which is asserted instead;
      below (wk1 taken from level k) and wsum_v (wsum * fsum for the per-column product) on every pair;
      top_read (w(nz) for +0 at the top level) can touch the rows of the top level alone, 1 / nzm of all rows: the cap is
        asserted over those rows, on every pair;
      multiply (a mask multiplied in) on a planted value tracer, on every pair;
      reverse (the columns walked backwards) over the rows of sums, except at nx = 2 where a sum of two terms has no order.
    The ties the ge variant turns on are planted by LD.make_plan_inputs; their share is asserted too."""
    ncrms, nx, nz = shape
    nzm = nz - 1
    inp = LD.make_plan_inputs(oracle, shape, 3, np.dtype(dtn).type, SEED)
    F, W = inp["f"], inp["w"]
    assert (W[:, :, -1] != 0).all() and np.abs(W[:, :, -1]).max() > 1
    Wq = W[:, :, :-1]
    b, i, k = np.indices(Wq.shape)
    quant = (Wq * 8 == np.round(Wq * 8))
    assert quant[(i + k) % 4 == 0].all() and (~quant[:, 2:nx + 2]).mean() >= 0.25
    up_ties, dn_ties = LD.tie_share(W, LD.WUP, LD.WDN)
    assert min(up_ties, dn_ties) >= (0.9 if nx >= 8 else 0.2), (up_ties, dn_ties)      # (nx < 8: every fourth row is planted)
    shares = {v: {} for v in LD.VARIANTS}
    for t, (wup, wdn) in enumerate(THR):
        acc = {v: [] for v in LD.VARIANTS}
        for j, (tc, first, ntr) in enumerate(TRIPLES[:4]):
            lo, hi = LC.call_args(F, tc, BOUNDS[(j + t) % 3], 60 + j)
            for v in LD.VARIANTS:
                if v == "top_read":
                    ref = LD.level_draft(F, W, tc, lo, hi, wup, wdn, first, ntr)
                    var = LD.level_draft(F, W, tc, lo, hi, wup, wdn, first, ntr, top_read=True)
                    top = lambda r: [None if a is None else a[:, -1:] for a in r]
                    acc[v].append(LD.share_differs(top(ref), top(var)))
                elif v == "reverse":
                    # (many columns in a class: else a sum has no order) no bounds, the class that holds most columns
                    ref = LD.level_draft(F, W, -1, None, None, wup, wdn, first, ntr)
                    var = LD.level_draft(F, W, -1, None, None, wup, wdn, first, ntr, reverse=True)
                    acc[v].append(LD.share_differs(ref[1:], var[1:]))
                else:
                    acc[v].append(LD.variant_share(v, F, W, tc, lo, hi, wup, wdn, first, ntr))
        for v in LD.VARIANTS:
            shares[v][(wup, wdn)] = float(np.mean(acc[v]))
    for (wup, wdn) in THR:
        key = (wup, wdn)
        both_inf = np.isinf(wup) and np.isinf(wdn)
        for v in ("ge", "swap"):
            assert (shares[v][key] == 0) if both_inf else (shares[v][key] >= 0.1), (v, key, shares[v])
        for v in ("below", "wsum_v", "top_read", "multiply"):
            assert shares[v][key] >= 0.1, (v, key, shares[v])
        assert shares["reverse"][key] == 0 if nx == 2 else shares["reverse"][key] >= 0.1, (key, shares["reverse"])


# ---- the plan model: the call changes nothing; the order of the checks
def _model(oracle, dtype=np.float64, T=3, shape=(5, 8, 6)):
    m = LD.PlanModelLevelDraft(oracle, *shape, T, dtype)
    return m, LD.make_plan_inputs(oracle, shape, T, dtype, 100)


def _state(m):
    return (m.boundary, m.uploaded, m.have_u, m.have_w, m.timing, m.ran, list(m.steps), list(m.fmax), list(m.flmax))


@pytest.mark.parametrize("boundary", [PM.GIVEN, PM.PERIODIC])
def test_plan_model_call_changes_no_array_and_no_mark(oracle, boundary):
    m, inp = _model(oracle)
    assert m.upload(inp) is None and m.set_boundary(boundary) is None and m.run() is None
    keep, state = {k: np.array(v) for k, v in m.a.items()}, _state(m)
    for j, (tc, first, ntr) in enumerate(TRIPLES):
        wup, wdn = THR[j % len(THR)]
        lo, hi = (None, None) if tc < 0 else LC.call_args(keep["f"][1:4], tc, BOUNDS[j % 3], 5)
        for kw in (dict(), dict(cnt=False), dict(fsum=False, wfsum=False), dict(cnt=False, wsum=False, fsum=False)):
            got = m.level_draft(tc, lo, hi, wup, wdn, first, ntr, sl0=1, n=3, **kw)
            want = LD.level_draft(keep["f"][1:4], keep["w"][1:4], tc, lo, hi, wup, wdn, first, ntr)
            for name, g, w_ in zip(("cnt", "wsum", "fsum", "wfsum"), got, want):
                assert (g is None) == (kw.get(name) is False)
                assert g is None or same(g, w_)
            assert _state(m) == state
            for k, v in keep.items():
                assert np.array_equal(bits(m.a[k]), bits(v)), k


def test_plan_model_check_order(oracle):
    """the error list of 3ac and its order"""
    m, inp = _model(oracle)
    lo = np.zeros((5, 5), np.float64, order="F")
    nan = float("nan")
    assert m.level_draft(0) == PM.ESTATE                                        # never filled
    assert m.level_draft(3) == PM.EINVAL and m.level_draft(-2) == PM.EINVAL     # ... the arguments come first
    assert m.upload(inp) is None
    state = _state(m)
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert m.level_draft(0, sl0=sl0, n=n) == PM.EINVAL, (sl0, n)
    for tc in (-2, 3, 9):
        assert m.level_draft(tc) == PM.EINVAL, tc
    assert m.level_draft(-1, lo) == PM.EINVAL and m.level_draft(-1, None, lo) == PM.EINVAL
    assert not isinstance(m.level_draft(-1), int) and not isinstance(m.level_draft(0), int)      # tc = -1; tc >= 0 without bounds
    assert m.level_draft(0, wup=nan) == PM.EINVAL and m.level_draft(0, wdn=nan) == PM.EINVAL
    assert m.level_draft(0, wup=-1.0, wdn=1.0) == PM.EINVAL and m.level_draft(0, wup=-INF, wdn=INF) == PM.EINVAL
    for wup, wdn in ((0.0, 0.0), (INF, -INF), (INF, INF), (-INF, -INF), (0.0, -0.0)):
        assert not isinstance(m.level_draft(0, wup=wup, wdn=wdn), int), (wup, wdn)
    assert m.level_draft(0, cnt=False, wsum=False, fsum=False, wfsum=False) == PM.EINVAL
    for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1)):
        assert m.level_draft(0, first=first, ntr=ntr) == PM.EINVAL, (first, ntr)
        assert m.level_draft(0, first=first, ntr=ntr, cnt=False, wsum=False, fsum=False) == PM.EINVAL      # wfsum alone asks too
        assert not isinstance(m.level_draft(0, first=first, ntr=ntr, fsum=False, wfsum=False), int)        # without sums: not looked at
    # the order: the range, the handle, tc, lo / hi without tc, the thresholds, the outputs, the tracers, the precision, the state
    assert m.level_draft(9, lo, None, nan, 0.0, 9, 9, sl0=0, n=0, cnt=False, wsum=False, fsum=False, wfsum=False, eb=4) == PM.EINVAL
    assert m.level_draft(0, eb=4) == PM.ESTATE                                  # a host form of the other precision
    assert m.level_draft(0, first=9, ntr=9, eb=4) == PM.EINVAL and m.level_draft(9, eb=4) == PM.EINVAL
    assert m.level_draft(0, wup=nan, eb=4) == PM.EINVAL and m.level_draft(-1, lo, eb=4) == PM.EINVAL
    m.multi = True
    assert m.level_draft(0) == PM.EUNSUPPORTED and m.level_draft(0, sl0=0, n=0) == PM.EINVAL
    assert m.level_draft(9, lo, None, nan, 0.0, 9, 9, cnt=False, wsum=False, fsum=False, wfsum=False) == PM.EUNSUPPORTED
    m.multi = False
    assert _state(m) == state
    # the plan must hold w: after run_uw MPDATA_ESTATE until w is imported whole again; u is not needed
    o = oracle.make_inputs(5, 8, 6, seed=7, dist=oracle.DIST_RAW_SIGNED)
    assert m.run_uw(o["u"], o["w"]) is None and not m.have_w
    assert m.level_draft(0) == PM.ESTATE and m.level_draft(9) == PM.EINVAL
    assert m.import_device({"u": o["u"]}) is None and m.level_draft(0) == PM.ESTATE
    m2, _ = _model(oracle)
    assert m2.upload(inp) is None and m2.run_uw(o["u"], o["w"]) is None
    assert m2.import_device({"w": inp["w"]}) is None and m2.have_w and not m2.have_u
    got = m2.level_draft(1, first=1, ntr=2)
    assert not isinstance(got, int)
    for g, w_ in zip(got, LD.level_draft(m2.a["f"], inp["w"], 1, None, None, LD.WUP, LD.WDN, 1, 2)):
        assert same(g, w_)


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.level_draft) and callable(mpdata.Plan.level_draft) and callable(mpdata.Plan.level_draft_host)
    for nm in ("level_draft", "level_draft_shapes"):
        assert nm in mpdata.__all__, nm
    assert mpdata.level_draft_shapes(5, 3, 8, 4) == {"lo": (7, 5), "hi": (7, 5), "cnt": (3, 7, 5), "wsum": (3, 7, 5), "fsum": (4, 3, 7, 5),
                                                     "wfsum": (4, 3, 7, 5)}
    assert mpdata.level_draft_shapes(2, 65, 239)["wfsum"] == (1, 3, 238, 2)


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [p.strip() for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3ac." in hdr
    sec = hdr.split("---- 3ac.")[1].split("---- 4.")[0]
    for word in ("tc", "lo", "hi", "wup", "wdn", "cnt", "wsum", "fsum", "wfsum", "first_tracer", "nx", "MPDATA_EUNSUPPORTED", "MPDATA_EINVAL",
                 "MPDATA_ESTATE", "UP", "DOWN", "ENV", "mpdata_plan_run_uw"):
        assert re.search(r"\b" + word + r"\b", sec), word
    for c, v in (("UP", 0), ("DOWN", 1), ("ENV", 2)):
        assert re.search(rf"#define MPDATA_LEVEL_DRAFT_{c} {v}\b", sec)
    assert "windowed plans" in sec.lower() and "are supported" in sec and "OWNED levels" in sec and "no seam refresh" in sec
    assert "rounded ONCE" in sec and "mpdata_plan_shard_plan" in sec and "compare-and-select" in sec and "never read" in sec
    assert "The plan must hold w" in sec and "u is not needed" in sec
    for line in ("wk1  = w(sl,i,k+1) for k < nzm,  +0 for k = nzm",
                 "a    = w(sl,i,k) + wk1 ;  wc = 0.5 * a",
                 "in_i = tc < 0 ? true : (lo ? c_i > lo(b,k) : true) and (hi ? c_i <= hi(b,k) : true)",
                 "class of column i, only where in_i:   UP (0): wc > wup    DOWN (1): wc < wdn    ENV (2): otherwise",
                 "cnt  (b,k,c)    :  q = +0;  do i = 1, nx:  if class_i == c:  q = q + 1",
                 "wsum (b,k,c)    :  s = +0;  do i = 1, nx:  if class_i == c:  s = s + wc",
                 "fsum (b,k,c,j)  :  s = +0;  do i = 1, nx:  if class_i == c:  s = s + v_i",
                 "wfsum(b,k,c,j)  :  s = +0;  do i = 1, nx:  if class_i == c:  p = wc * v_i;  s = s + p"):
        assert line in sec, line
    # the three bit relations
    assert "bits of 3v's cnt and csum" in sec and "bits of 3g's sum" in sec and "equals 3v's cnt" in sec
    assert hdr.index("---- 3ab.") < hdr.index("---- 3ac.") < hdr.index("---- 4.")


def test_library_exports_and_ctypes_agree_with_the_header(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*", ctypes.c_double: "double"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)
    names = lambda n: [re.split(r"[\s*]+", p)[-1] for p in _c_params(hdr, n)]
    assert names("mpdata_plan_level_draft_device") == ["plan", "sl0", "n", "tc", "lo", "hi", "wup", "wdn", "cnt", "wsum", "fsum", "wfsum",
                                                       "first_tracer", "ntracers"]
    assert names("mpdata_plan_level_draft") == names("mpdata_plan_level_draft_f32") == \
        ["plan", "sl0", "n", "tc", "lo", "hi", "wup", "wdn", "cnt", "wsum", "fsum", "wfsum"]
    assert names("mpdata_level_draft_device") == names("mpdata_level_draft_f32_device") == \
        ["ncrms", "nx", "nz", "ntracers", "sl0", "n", "f", "w", "tc", "lo", "hi", "wup", "wdn", "cnt", "wsum", "fsum", "wfsum", "first_tracer",
         "ntr", "stream"]
    for k in (6, 7, 9, 10):                                  # f, w, lo and hi are only read
        assert _c_params(hdr, "mpdata_level_draft_device")[k].startswith("const "), k
    for n in NAMES:                                          # the thresholds: doubles by value in every form
        assert [p for p in _c_params(hdr, n) if p.endswith("wup") or p.endswith("wdn")] == ["double wup", "double wdn"], n


@pytest.mark.parametrize("name", NAMES)
def test_fortran_interface_agrees_with_the_header(name):
    """every interface, bound by the literal name, public, the dummy arguments in the header's order, each of the header's
    kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function " + name + r"_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"" + name + r"\"\)(.*?)end function",
                  f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, name)
    cargs = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert fargs == cargs, (fargs, cargs)
    decl = {}
    for line in m.group(2).splitlines():
        d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\)|real\(c_double\))\s*,\s*value\s*::\s*(.*)", line)
        if d:
            for a in d.group(2).split(","):
                decl[a.strip()] = d.group(1)
    for p, a in zip(params, cargs):
        want = "type(c_ptr)" if "*" in p else "integer(c_int64_t)" if p.startswith("int64_t ") else \
            "real(c_double)" if p.startswith("double ") else "integer(c_int)"
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert re.search(r"public ::.*\b" + name + r"_c\b", f90)
    # in the second interface block, behind 3ab's bindings
    assert f90.index("mpdata_level_hist_f32_device_c(ncrms") < f90.index(name + "_c(")
    assert f90.count("\n  interface\n") == 2 and f90.rindex("\n  interface\n") < f90.index(name + "_c(")
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "level_draft_calls.F90"))
    mk = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "Makefile")).read()
    assert re.search(r"^CALLS = .*\blevel_draft\b", mk, re.M)


def test_argument_errors_without_device(mpdata):
    """every refusal that needs no plan, in the stated order: sizes, the block, w, f where it is needed, tc, lo / hi without
    tc, the thresholds, the outputs, the tracers"""
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    err = L.mpdata_last_error
    nan = float("nan")
    for fn in (L.mpdata_level_draft_device, L.mpdata_level_draft_f32_device):
        call = lambda ncrms=4, nx=5, nz=6, T=3, sl0=0, n=4, f=one, w=one, tc=0, lo=one, hi=None, wup=0.25, wdn=-0.25, cnt=one, wsum=None, \
            fsum=one, wfsum=None, first=0, ntr=3: fn(ncrms, nx, nz, T, sl0, n, f, w, tc, lo, hi, wup, wdn, cnt, wsum, fsum, wfsum, first, ntr, None)
        assert call(nx=0) == mpdata.EINVAL
        assert call(nz=1) == mpdata.EINVAL and b"nz=1" in err()
        assert call(ncrms=0) == mpdata.EINVAL and call(T=0) == mpdata.EINVAL
        for sl0, n in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(sl0=sl0, n=n) == mpdata.EINVAL and b"outside" in err(), (sl0, n)
        assert call(w=None) == mpdata.EINVAL and b"null w" in err()
        assert call(f=None) == mpdata.EINVAL and b"null f" in err()
        assert call(f=None, tc=-1, lo=None) == mpdata.EINVAL and b"null f" in err()                  # fsum reads f
        assert call(f=None, fsum=None) == mpdata.EINVAL and b"null f" in err()                       # the condition reads f
        assert call(f=None, tc=-1, lo=None, fsum=None, wfsum=one) == mpdata.EINVAL and b"null f" in err()
        for tc in (-2, 3):
            assert call(tc=tc) == mpdata.EINVAL and b"condition tracer" in err(), tc
        assert call(tc=-1) == mpdata.EINVAL and b"without a condition tracer" in err()
        assert call(tc=-1, lo=None, hi=one) == mpdata.EINVAL and b"without a condition tracer" in err()
        assert call(wup=nan) == mpdata.EINVAL and b"NaN" in err() and call(wdn=nan) == mpdata.EINVAL and b"NaN" in err()
        assert call(wup=0.0, wdn=0.5) == mpdata.EINVAL and b"wdn" in err()
        assert call(wup=-INF, wdn=INF) == mpdata.EINVAL and b"wdn" in err()
        assert call(cnt=None, fsum=None) == mpdata.EINVAL and b"all NULL" in err()
        for first, ntr in ((0, 0), (-1, 2), (0, 4), (3, 1), (2, 2), (0, -1), (2147483647, 2)):
            assert call(first=first, ntr=ntr) == mpdata.EINVAL and b"tracer range" in err(), (first, ntr)
            assert call(first=first, ntr=ntr, fsum=None, wfsum=one) == mpdata.EINVAL and b"tracer range" in err()
        # the order: each refusal hides the ones behind it
        assert call(nz=1, sl0=9, w=None, f=None, tc=9, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"nz=1" in err()
        assert call(sl0=9, w=None, f=None, tc=9, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"outside" in err()
        assert call(w=None, f=None, tc=9, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"null w" in err()
        assert call(f=None, tc=9, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"null f" in err()
        assert call(tc=9, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"condition tracer" in err()
        assert call(tc=-1, wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"without a condition" in err()
        assert call(wup=nan, cnt=None, fsum=None) == mpdata.EINVAL and b"NaN" in err()
        assert call(wup=-1.0, wdn=1.0, cnt=None, fsum=None, ntr=9) == mpdata.EINVAL and b"wdn" in err()
        assert call(cnt=None, fsum=None, ntr=9) == mpdata.EINVAL and b"all NULL" in err()
        assert call(cnt=None, ntr=9) == mpdata.EINVAL and b"tracer range" in err()
    dev = lambda plan=one, sl0=0, n=1, tc=0, wup=0.25, cnt=one: \
        L.mpdata_plan_level_draft_device(plan, sl0, n, tc, None, None, wup, -0.25, cnt, None, None, None, 0, 0)
    assert dev(plan=None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_draft(None, 0, 1, 0, None, None, 0.25, -0.25, one, None, None, None) == mpdata.EINVAL and b"null plan" in err()
    assert L.mpdata_plan_level_draft_f32(None, 0, 1, 0, None, None, 0.25, -0.25, one, None, None, None) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert dev(sl0=sl0, n=n) == mpdata.EINVAL
    assert dev(n=0, tc=9, wup=nan, cnt=None) == mpdata.EINVAL and b"n = 0" in err()     # the range came first


def test_new_kernels_do_not_spill_and_use_no_lds():
    """the resource-usage report the build writes next to the object of mpdata_level_draft.hip: no scratch memory, no vector
    and no scalar register spilled and no static LDS in any kernel; the file asks for no dynamic LDS and has no barrier and
    no atomic.  Kernels: the plan-layout one with double and float2 elements, with and without wfsum, and the
    reference-layout one for double and float."""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_level_draft.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*wm_level_draft_kernel", txt)) == 4
    assert len(re.findall(r"Function Name: \S*ref_level_draft_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 6 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}
    assert set(re.findall(r"Dynamic Stack: (\w+)", txt)) == {"False"}
    src = open(os.path.join(csrc, "mpdata_level_draft.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "__shared__" not in code and "__syncthreads" not in code and "atomic" not in code and "#ifndef" not in code
    assert "getenv" not in code and "__shfl" not in code
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_level_draft\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,mpdata_level_draft", mk)
    assert "mpdata_level_draft$(O)" in mk.split("OBJS :=")[1].split("\n")[0]
    assert "mpdata_level_draft.hip" in open(os.path.join(csrc, "mpdata_wm_walk.h")).read().split("#ifndef")[0]
