"""GPU tests of the level statistics of a resident plan (include/mpdata_hip.h 3g): mpdata_plan_level_stats_device, the
host forms, the array forms and their Python face Plan.level_stats / level_stats_host / level_stats.

Every comparison is bit for bit (util.assert_bitwise) against the numpy model of tests/level_stats_model.py -- an
explicit loop over i in the array's dtype -- applied to a reference-layout truth:
  (a) after the upload: the uploaded f;
  (b) after one run of an EXACT plan: the CPU oracle's f (the plan's f is bit-identical to it);
  (c) FAST plans, periodic runs, run_uw, block imports, call sequences: the plan's own whole export (existing code; the
      feature under test is the reduction, not the advection).
Every truth is asserted to hold no -0.0 (the sign of a zero min / max is unspecified).  Every output lies inside a larger
buffer with a patterned band of 4 KiB on both sides that must come back unchanged.

Column chunks (slp * nzm * 8 bytes, tests ids): nz 3 and 5 are whole 128-byte lines (128, 256 bytes: the remainder part
is empty); nz 12, 28, 58, 72, 130 have both parts (352, 432, 456, 568, 1032 bytes).  A chunk shorter than a line does
not exist: plan creation refuses one (the two-instructions-per-fetch invariant of the plan kernels)."""
import ctypes

import numpy as np
import pytest

import level_stats_model as LM
from plan_harness import BAND, _defaults, banded, tdt, upload
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu


def chunk_kind(nz, dt=np.float64):
    b = (LM._tile(nz, dt) // (2 if dt == np.float32 else 1)) * (nz - 1) * 8
    return f"chunk{b}B-" + ("whole-lines" if b % 128 == 0 else "lines+rest")


def new_plan(M, name, variant=None, ref=False, tall=False, odd=False, **kw):
    """the plan of LM.INPUTS[name] and its inputs; ref / tall / odd: the switches of the kind"""
    shape, T, dt, seed = LM.INPUTS[name]
    M.set_variant(M.VARIANT_EXACT if variant is None else variant)
    M.set_plan_layout(M.LAYOUT_REFERENCE if ref else M.LAYOUT_WAVEMAJOR)
    M.set_tall_columns(int(tall))
    M.set_f32_odd_ncrms(int(odd))
    return M.Plan(*shape, T, dtype=dt, **kw)


def stats(p, dt, nzm, sl0, n, first=0, ntr=None, which=("sum", "min", "max")):
    """Plan.level_stats into banded buffers -> {name: Fortran array (n, nzm[, ntr])}; the bands are checked"""
    import torch
    shape = (() if ntr is None else (ntr,)) + (nzm, n)
    bufs = {k: banded(shape, dt) for k in which}
    torch.cuda.synchronize()      # (the plan may run on a stream that does not wait for the one that filled the buffers)
    p.level_stats(sl0, n, first_tracer=first, **{k: v[2] for k, v in bufs.items()})
    p.sync()
    out = {}
    for k, (raw, orig, view) in bufs.items():
        assert torch.equal(raw[:BAND], orig[:BAND]) and torch.equal(raw[-BAND:], orig[-BAND:]), f"{k}: a band byte changed"
        out[k] = to_host(view)
    return out


def model(F):
    interior = np.asarray(F)[:, 3:-3]
    assert not LM.has_negative_zero(interior) and np.all(np.isfinite(interior))
    return dict(zip(("sum", "min", "max"), LM.level_stats(F)))


def same(got, want, what):
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def whole_export(M, p, name):
    import torch
    shape, T, dt, _ = LM.INPUTS[name]
    f = torch.empty(M.shapes(*shape, T)["f"], dtype=tdt(dt), device="cuda:0")
    p.export_device(f=f)
    p.sync()
    return to_host(f)


def check_whole(M, p, name, F, what):
    shape, T, dt, _ = LM.INPUTS[name]
    same(stats(p, dt, shape[2] - 1, 0, shape[0], 0, None if T == 1 else T), model(F), f"{name} {what}")


# ---- 1. every kind of plan, every state
KINDS = [(f"f64-nz{nz}", {}, chunk_kind(nz)) for nz in (3, 5, 12, 28, 58, 72, 130)] + \
        [(f"f64-nx{nx}", {}, "") for nx in (1, 2, 5, 32)] + \
        [(f"f32-nz{nz}-even", {}, chunk_kind(nz, np.float32)) for nz in (5, 28, 72)] + \
        [(f"f32-nz{nz}-odd", dict(odd=True), "phantom") for nz in (5, 28, 72)] + \
        [("f32-nz12-odd-ref", {}, "reference-layout"), ("f64-nz12-ref", dict(ref=True), ""), ("f32-nz12-ref", dict(ref=True), ""),
         ("f64-tall", dict(tall=True), "windowed"), ("f32-tall-odd", dict(tall=True, odd=True), "windowed-phantom"),
         ("f64-tall-kmarch", {}, "reference-layout")]


@pytest.mark.parametrize("name,sw,note", KINDS, ids=[f"{k}{'-' + n if n else ''}" for k, _, n in KINDS])
def test_every_plan_kind_and_state(mpdata, oracle, name, sw, note):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    want_layout = M.LAYOUT_REFERENCE if (sw.get("ref") or "reference-layout" in note) else M.LAYOUT_WAVEMAJOR
    assert p.layout == want_layout and (p.level_windows > 1) == bool(sw.get("tall"))
    upload(p, inp)
    check_whole(M, p, name, inp["f"], "(a) after the upload")
    p.run()
    check_whole(M, p, name, oracle.advect(inp)[0], "(b) after one EXACT run")
    # (c) from here on: two periodic runs (the stats call reads no halo and wraps nothing), run_uw, a block import that
    # replaces the plan's last instance
    p.set_boundary(M.BOUNDARY_PERIODIC)
    p.run()
    p.run()
    got = stats(p, dt, nz - 1, 0, ncrms, 0, None if T == 1 else T)     # while the halos are stale
    same(got, model(whole_export(M, p, name)), f"{name} (c) after two periodic runs")
    p.set_boundary(M.BOUNDARY_GIVEN)
    other = LM.make(oracle, shape, T, dt, seed + 50)
    p.run_uw(to_dev(other["u"]), to_dev(other["w"]))
    check_whole(M, p, name, whole_export(M, p, name), "(c) after run_uw")
    p.import_block(ncrms - 1, f=to_dev(np.asfortranarray(other["f"][ncrms - 1:])))
    F = whole_export(M, p, name)
    assert_bitwise(F[ncrms - 1:], other["f"][ncrms - 1:], "the imported block")
    check_whole(M, p, name, F, "(c) after a block import of the last instance")
    p.close()
    # FAST: (a) and (c)
    p = new_plan(M, name, variant=M.VARIANT_FAST, **sw)
    upload(p, inp)
    check_whole(M, p, name, inp["f"], "FAST (a) after the upload")
    p.run()
    check_whole(M, p, name, whole_export(M, p, name), "FAST (c) after one run")
    p.close()


# ---- 2. blocks: odd starts and ends that split fp32 pairs and tiles
BLOCKS = ((0, 11), (0, 1), (10, 1), (3, 5), (1, 9))


@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-tall-blocks", dict(tall=True)),
                                     ("f32-tall-blocks", dict(tall=True, odd=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_blocks_are_slices_of_the_whole(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert ncrms == 11
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    upload(p, inp)
    p.run()
    ntr = None if T == 1 else T
    W = stats(p, dt, nz - 1, 0, ncrms, 0, ntr)
    same(W, model(oracle.advect(inp)[0]), f"{name} whole")
    for sl0, n in BLOCKS:
        got = stats(p, dt, nz - 1, sl0, n, 0, ntr)
        same(got, {k: np.asfortranarray(v[sl0:sl0 + n]) for k, v in W.items()}, f"{name} block {sl0, n}")
    p.close()


# ---- 3. tracers: all three, and the sub-range first = 1, count = 2
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-nz12-ref", dict(ref=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_tracer_ranges(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert T == 3
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    want = model(inp["f"])
    same(stats(p, dt, nz - 1, 0, ncrms, 0, 3), want, f"{name} all tracers")
    same(stats(p, dt, nz - 1, 0, ncrms, 1, 2), {k: np.asfortranarray(v[..., 1:3]) for k, v in want.items()}, f"{name} tracers 1..2")
    same(stats(p, dt, nz - 1, 2, 7, 2, None), {k: np.asfortranarray(v[2:9, :, 2]) for k, v in want.items()}, f"{name} tracer 2, a block")
    assert pytest.raises(M.MpdataError, stats, p, dt, nz - 1, 0, ncrms, 2, 2).value.code == M.EINVAL
    p.close()


# ---- 4. outputs: a NULL output is skipped, each single output alone gives the same bits
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-nz12-ref", dict(ref=True)),
                                     ("f64-tall-blocks", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_single_outputs(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name, **sw)
    upload(p, LM.make(oracle, shape, T, dt, seed))
    ntr = None if T == 1 else T
    for sl0, n in ((0, ncrms), (3, 5)):
        all3 = stats(p, dt, nz - 1, sl0, n, 0, ntr)
        for which in (("sum",), ("min",), ("max",), ("sum", "max")):
            got = stats(p, dt, nz - 1, sl0, n, 0, ntr, which=which)
            assert set(got) == set(which)
            same(got, all3, f"{name} {which} alone, block {sl0, n}")
    with pytest.raises(M.MpdataError) as e:
        p.level_stats(0, ncrms)
    assert e.value.code == M.EINVAL
    assert M.lib().mpdata_plan_level_stats_device(p._p, 0, ncrms, None, None, None, 0, 1) == M.EINVAL
    p.close()


# ---- 5. the array forms, on a stream of their own
@pytest.mark.parametrize("name", ["f64-array", "f32-array"])
def test_array_forms(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    assert (shape, T) == ((7, 5, 6), 2)
    ncrms, nx, nz = shape
    F = LM.make(oracle, shape, T, dt, seed)["f"]
    want = model(F)
    f = to_dev(F)
    keep = f.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    bufs = {k: banded((T, nz - 1, ncrms), dt) for k in ("sum", "min", "max")}
    M.level_stats(f, stream=s, **{k: v[2] for k, v in bufs.items()})
    s.synchronize()
    same({k: to_host(v[2]) for k, v in bufs.items()}, want, name)
    for k, (raw, orig, _) in bufs.items():
        assert torch.equal(raw[:BAND], orig[:BAND]) and torch.equal(raw[-BAND:], orig[-BAND:]), k
    assert torch.equal(f, keep)
    only = banded((T, nz - 1, ncrms), dt)
    M.level_stats(f, min=only[2])                       # the current stream, one output
    torch.cuda.synchronize()
    assert_bitwise(to_host(only[2]), want["min"], f"{name} min alone")
    one = to_dev(np.asfortranarray(F[..., 1]))          # a 3-d f: one tracer, 2-d outputs
    o = banded((nz - 1, ncrms), dt)
    M.level_stats(one, sum=o[2])
    torch.cuda.synchronize()
    assert_bitwise(to_host(o[2]), np.asfortranarray(want["sum"][..., 1]), f"{name} one tracer")


# ---- 6. the host forms
@pytest.mark.parametrize("name,sw", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f32-nz12-ref", dict(ref=True)),
                                     ("f64-tall", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_host_forms(mpdata, oracle, name, sw):
    M = mpdata
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, **sw)
    upload(p, inp)
    want = model(inp["f"])
    for sl0, n in ((0, ncrms), (1, ncrms - 2), (ncrms - 1, 1)):     # (the staging buffer grows and is reused)
        host = {k: np.full((n, nz - 1) + ((T,) if T > 1 else ()), -7, dt, order="F") for k in ("sum", "min", "max")}
        p.level_stats_host(sl0, n, **host)
        same(host, {k: np.asfortranarray(v[sl0:sl0 + n]) for k, v in want.items()}, f"{name} host {sl0, n}")
        m = np.full_like(host["max"], -7)
        p.level_stats_host(sl0, n, max=m)
        assert_bitwise(m, host["max"], f"{name} host max alone")
    # the form of the other precision
    other = np.float32 if dt == np.float64 else np.float64
    a = np.zeros((ncrms, nz - 1) + ((T,) if T > 1 else ()), other, order="F")
    fn = M.lib().mpdata_plan_level_stats_f32 if dt == np.float64 else M.lib().mpdata_plan_level_stats
    assert fn(p._p, 0, ncrms, ctypes.c_void_p(a.ctypes.data), None, None) == M.ESTATE
    assert not a.any()
    assert M.lib().mpdata_plan_level_stats(p._p, 0, ncrms, None, None, None) == M.EINVAL
    p.close()


# ---- 7. errors
def _code(M, fn, *a, **kw):
    with pytest.raises(M.MpdataError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    p = new_plan(M, name)
    out = torch.zeros((T, nz - 1, ncrms), dtype=torch.float64, device="cuda:0")
    assert _code(M, p.level_stats, 0, ncrms, sum=out) == M.ESTATE            # never filled
    h = np.zeros((ncrms, nz - 1, T), order="F")
    assert _code(M, p.level_stats_host, 0, ncrms, sum=h) == M.ESTATE
    upload(p, LM.make(oracle, shape, T, dt, seed))
    p.level_stats(0, ncrms, sum=out)
    ptr = ctypes.c_void_p(out.data_ptr())
    L = M.lib()
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert L.mpdata_plan_level_stats_device(p._p, sl0, n, ptr, None, None, 0, 1) == M.EINVAL, (sl0, n)
    for first, cnt in ((-1, 1), (0, 0), (0, T + 1), (T, 1)):
        assert L.mpdata_plan_level_stats_device(p._p, 0, ncrms, ptr, None, None, first, cnt) == M.EINVAL, (first, cnt)
    p.sync()
    assert not torch.isnan(out).any()
    p.close()


def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-blocks"
    shape, T, dt, seed = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = LM.make(oracle, shape, T, dt, seed)
    p = new_plan(M, name, devices=[0, 0])
    upload(p, inp)
    want = model(inp["f"])
    assert _code(M, stats, p, dt, nz - 1, 0, ncrms, 0, T) == M.EUNSUPPORTED
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    h = np.zeros((ncrms, nz - 1, T), order="F")
    assert _code(M, p.level_stats_host, 0, ncrms, sum=h) == M.EUNSUPPORTED
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        same(stats(q, dt, nz - 1, 0, nloc, 0, T), {k: np.asfortranarray(v[s0:s0 + nloc]) for k, v in want.items()}, f"shard {g}")
        same(stats(q, dt, nz - 1, 1, 3, 0, T), {k: np.asfortranarray(v[s0 + 1:s0 + 4]) for k, v in want.items()}, f"shard {g} block")
        q.close()
    p.close()


# ---- 8. a seeded call sequence (oracle/plan_model.py): the stats of every state, and no state changed
@pytest.mark.parametrize("kind", ["wm32", "ref", "f32-odd-28", "tall-239", "tall-f32-odd-239"])
def test_call_sequence_states_and_no_state_change(mpdata, oracle, kind):
    """Plays sequence SEEDS[kind][0] twice on EXACT plans -- as tests/test_plan_sequences.py does, and with a whole-plan host
    call and a block device call of the statistics behind every op that succeeds -- and compares: the statistics with the
    model applied to the plan model's f (EXACT: the plan's f is bit-identical to it, which the plain play asserts), and
    every return code and every array read back by the two plays with each other."""
    from oracle import plan_model as PM
    from test_plan_sequences import Player
    M = mpdata
    seed = PM.SEEDS[kind][0]
    ops = PM.sequences(kind, seed, PM.LENGTH, oracle)

    class StatsPlayer(Player):
        calls = 0

        def do(self, i, op, want):
            super().do(i, op, want)
            m = self.model
            if not m.uploaded:
                return
            T, nzm, dt = self.T, self.nz - 1, self.dt
            F = m.a["f"] if T > 1 else m.a["f"][..., 0]
            wantS = model(F)
            host = {k: np.full((self.ncrms, nzm) + ((T,) if T > 1 else ()), -7, dt, order="F") for k in ("sum", "min", "max")}
            self.p.level_stats_host(0, self.ncrms, **host)
            same(host, wantS, f"op {i} {op['op']}: whole-plan host call")
            sl0 = i % self.ncrms
            n = min(2, self.ncrms - sl0)
            got = stats(self.p, dt, nzm, sl0, n, 0, None if T == 1 else T)
            same(got, {k: np.asfortranarray(v[sl0:sl0 + n]) for k, v in wantS.items()}, f"op {i} {op['op']}: block {sl0, n}")
            StatsPlayer.calls += 1

    def play(cls):
        pl = cls(M, oracle, kind, "exact")
        try:
            pl.check_kind()
            pl.play([dict(op) for op in ops])    # (errors are asserted against the model's codes inside)
        finally:
            pl.p.close()
        return pl.got

    plain, with_stats = play(Player), play(StatsPlayer)
    assert StatsPlayer.calls >= PM.LENGTH // 2
    assert plain.keys() == with_stats.keys() and len(plain) >= 3
    for i in plain:
        assert plain[i].keys() == with_stats[i].keys()
        for k in plain[i]:
            assert_bitwise(plain[i][k], with_stats[i][k], f"op {i}: {k} read back with and without the stats calls")
