"""GPU tests of the per-instance scaling of a resident plan's velocities (include/mpdata_hip.h 3j):
mpdata_plan_scale_uw_device, the host forms, the array forms and their Python face Plan.scale_uw / scale_uw_host /
scale_uw.

A plan's u and w have no export, so what the call did shows in what reads them: a run (f and flux, bit for bit against
the CPU oracle on the numpy-scaled u, w: an EXACT plan is bit-identical to it) and the Courant number (clev and cinst
against tests/courant_model.py on them).  Every comparison is bit for bit (util.assert_bitwise) but the one FAST run,
which is held to the README's bound.  The model is tests/scale_uw_model.py -- the factor broadcast over the column and
level axes in the array's dtype; the first factors applied to an uploaded u, w are the ones the guard of
tests/test_scale_uw_cpu.py covers (every instance with a factor that is not 1 shows in f and in cinst, u's and w's
scaling each on its own).  The factors lie inside a larger buffer with a patterned band of 4 KiB on both sides; the
bands and the factors must come back unchanged.

The plan kinds, blocks and shapes are those of tests/test_plan_level_stats.py (LM.INPUTS)."""
import ctypes

import numpy as np
import pytest

import courant_model as CM
import level_stats_model as LM
import plan_harness as H
import scale_uw_model as SM
from oracle import plan_model as PM
from plan_harness import BAND, _defaults, banded, upload
from test_plan_courant import cour
from test_plan_level_add import same_as_model
from test_plan_level_stats import BLOCKS, KINDS, _code, new_plan
from test_plan_tall_columns import C_FAST, UNIT
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu
BLOCK_INPUTS = [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f64-tall-blocks", dict(tall=True)),
                ("f32-tall-blocks", dict(tall=True, odd=True))]


def dev_s(s):
    """host factors (n,) or None -> (raw, pristine copy, device view (n,)) between two bands, or None"""
    import torch
    if s is None:
        return None
    raw, _, view = banded(s.shape, s.dtype)
    view.copy_(torch.from_numpy(s))
    torch.cuda.synchronize()
    return raw, raw.clone(), view


def scale(p, su=None, sw=None, sl0=0, n=None):
    """Plan.scale_uw of banded factors; afterwards the bands and the factors are as they were"""
    import torch
    bu, bw = dev_s(su), dev_s(sw)
    p.scale_uw(None if bu is None else bu[2], None if bw is None else bw[2], sl0, n)
    p.sync()
    for k, b in (("su", bu), ("sw", bw)):
        assert b is None or torch.equal(b[0], b[1]), f"a byte of {k} or of its bands changed"


def model_of(oracle, name, inp):
    shape, T, dt, _ = LM.INPUTS[name]
    m = SM.PlanModelScale(oracle, *shape, T, dt)
    assert m.upload(inp) is None
    return m


def run_equals_oracle(M, oracle, p, name, inp, u, w, what):
    """one EXACT run of the plan: f and flux = the oracle on reference-layout u, w"""
    nzm = LM.INPUTS[name][0][2] - 1
    p.run()
    f2, fl2 = oracle.advect(dict(inp, u=u, w=w))
    got = H.whole(M, p, LM.INPUTS[name])
    assert_bitwise(got["f"].reshape(f2.shape, order="F"), f2, f"{name} {what}: f")
    assert_bitwise(got["flux"].reshape(fl2.shape, order="F")[:, :nzm], fl2[:, :nzm], f"{name} {what}: flux")
    return f2


def courant_equals_model(p, name, inp, u, w, what, sl0=0, n=None):
    shape, _, dt, _ = LM.INPUTS[name]
    n = shape[0] - sl0 if n is None else n
    clev, cinst = CM.courant(u, w, inp["rho"], inp["adz"])
    got = cour(p, dt, shape[2] - 1, sl0, n)
    assert_bitwise(got["clev"], np.asfortranarray(clev[sl0:sl0 + n]), f"{name} {what}: clev")
    assert_bitwise(got["cinst"], np.ascontiguousarray(cinst[sl0:sl0 + n]), f"{name} {what}: cinst")


# ---- 1. every kind of plan
@pytest.mark.parametrize("name,sw_,note", KINDS, ids=[f"{k}{'-' + n if n else ''}" for k, _, n in KINDS])
def test_every_plan_kind(mpdata, oracle, name, sw_, note):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = SM.make(oracle, name)
    su, sw = SM.s_like(name)
    u2, w2 = SM.scale_uw(inp["u"], inp["w"], su, sw)
    # (a) upload -> both factors -> the Courant number and one EXACT run
    p = new_plan(M, name, **sw_)
    want_layout = M.LAYOUT_REFERENCE if (sw_.get("ref") or "reference-layout" in note) else M.LAYOUT_WAVEMAJOR
    assert p.layout == want_layout and (p.level_windows > 1) == bool(sw_.get("tall"))
    upload(p, inp)
    scale(p, su, sw)
    courant_equals_model(p, name, inp, u2, w2, "(a) upload, su and sw")
    f_exact = run_equals_oracle(M, oracle, p, name, inp, u2, w2, "(a) upload, su and sw, run")
    p.close()
    # (b) only su, only sw, on fresh plans
    for a, b, what in ((su, None, "only su"), (None, sw, "only sw")):
        p = new_plan(M, name, **sw_)
        upload(p, inp)
        scale(p, a, b)
        run_equals_oracle(M, oracle, p, name, inp, u2 if a is not None else inp["u"], w2 if b is not None else inp["w"], f"(b) {what}, run")
        p.close()
    # (c) PERIODIC: run, scale, run against the plan model; GIVEN: run_uw, after which the plan holds neither array
    p = new_plan(M, name, **sw_)
    upload(p, inp)
    m = model_of(oracle, name, inp)
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert m.set_boundary(PM.PERIODIC) is None
    p.run()
    assert m.run() is None
    su1, sw1 = SM.s_like(name, 1)
    scale(p, su1, sw1)
    assert m.scale_uw(su1, sw1) is None
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "(c) periodic: run, scale, run")
    p.set_boundary(M.BOUNDARY_GIVEN)
    assert m.set_boundary(PM.GIVEN) is None
    ou, ow = SM.other(oracle, name)
    p.run_uw(to_dev(ou), to_dev(ow))
    assert m.run_uw(ou, ow) is None
    du, dw = dev_s(su), dev_s(sw)
    for a, b, ma, mb in ((du[2], dw[2], su, sw), (du[2], None, su, None), (None, dw[2], None, sw)):
        assert _code(M, p.scale_uw, a, b) == M.ESTATE == m.scale_uw(ma, mb)
    assert b"does not hold" in M.lib().mpdata_last_error()
    same_as_model(M, p, name, m, "(c) after run_uw and the refused calls")
    last = dict(u=np.asfortranarray(ou[ncrms - 1:]), w=np.asfortranarray(ow[ncrms - 1:]))
    assert _code(M, p.import_block, ncrms - 1, u=to_dev(last["u"]), w=to_dev(last["w"])) == M.ESTATE == m.import_block(ncrms - 1, 1, last)
    assert _code(M, p.scale_uw, du[2], dw[2]) == M.ESTATE == m.scale_uw(su, sw)
    assert _code(M, p.scale_uw, du[2], dw[2], ncrms - 1, 1) == M.EINVAL                 # (a (1,) block needs (1,) factors)
    assert _code(M, p.scale_uw, du[2][:1], dw[2][:1], ncrms - 1, 1) == M.ESTATE == m.scale_uw(su[:1], sw[:1], ncrms - 1, 1)
    same_as_model(M, p, name, m, "(c) after the refused block import")
    p.close()
    # FAST: the same bits in u, w (the Courant number), and a run within the README's bound of the EXACT result
    p = new_plan(M, name, variant=M.VARIANT_FAST, **sw_)
    upload(p, inp)
    scale(p, su, sw)
    courant_equals_model(p, name, inp, u2, w2, "FAST upload, su and sw")
    p.run()
    got = H.whole(M, p, LM.INPUTS[name], ("f",))["f"].reshape(f_exact.shape, order="F")
    fin = inp["f"].reshape(got.shape, order="F")
    for t in range(T):
        sel = (Ellipsis, t) if T > 1 else Ellipsis
        S = float(np.max(np.abs(fin[sel].astype(np.float64))))
        d = float(np.max(np.abs(got[sel].astype(np.float64) - f_exact[sel].astype(np.float64))))
        print(f"{name} FAST run tracer {t}: max|df| = {d / (UNIT[dt] * S):.2f} u max|f_in|")
        assert d <= C_FAST * UNIT[dt] * S, f"{name} FAST tracer {t}: max|df| = {d:.3e} > 64 u * {S:.3e}"
    p.close()


# ---- 2. blocks: odd starts and ends that split fp32 pairs and tiles
@pytest.mark.parametrize("name,sw_", BLOCK_INPUTS, ids=lambda v: v if isinstance(v, str) else "")
def test_blocks_leave_the_rest_alone(mpdata, oracle, name, sw_):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    assert ncrms == 11
    inp = SM.make(oracle, name)
    p = new_plan(M, name, **sw_)
    assert p.layout == M.LAYOUT_WAVEMAJOR
    upload(p, inp)
    dev = {k: to_dev(inp[k]) for k in ("f", "u", "w", "flux")}

    def refill():
        p.import_device(**dev)

    def scaled(blocks, k=0):
        """reference-layout u, w with the k-th factors applied to the instances of `blocks`"""
        u, w = np.array(inp["u"], order="F"), np.array(inp["w"], order="F")
        for sl0, n in blocks:
            su, sw = SM.s_like(name, k, sl0, n)
            u[sl0:sl0 + n], w[sl0:sl0 + n] = SM.scale_uw(u[sl0:sl0 + n], w[sl0:sl0 + n], su, sw)
        return u, w

    for sl0, n in BLOCKS:
        refill()
        scale(p, *SM.s_like(name, 0, sl0, n), sl0, n)
        u, w = scaled([(sl0, n)])
        # a wrongly scaled split-pair partner, tile neighbour or padding slot shows here; on the odd fp32 plans the
        # phantom half followed instance 10 where the block holds it: the run matches the oracle for EVERY instance
        courant_equals_model(p, name, inp, u, w, f"block {sl0, n}")
        run_equals_oracle(M, oracle, p, name, inp, u, w, f"block {sl0, n}, run")
    # one array of a block alone: the other array's instances keep their bits
    refill()
    su, sw = SM.s_like(name, 0, 3, 5)
    scale(p, su, None, 3, 5)
    scale(p, None, np.ascontiguousarray(sw[1:3]), 4, 2)
    u, w = np.array(inp["u"], order="F"), np.array(inp["w"], order="F")
    u[3:8] = SM.scale_uw(u[3:8], w[3:8], su, None)[0]
    w[4:6] = SM.scale_uw(u[4:6], w[4:6], None, np.ascontiguousarray(sw[1:3]))[1]
    run_equals_oracle(M, oracle, p, name, inp, u, w, "su on (3, 5), sw on (4, 2), run")
    # two disjoint blocks that cover the plan (they split the pair (4, 5)), one after the other = one whole-plan call
    refill()
    for sl0, n in ((5, 6), (0, 5)):
        scale(p, *SM.s_like(name, 1, sl0, n), sl0, n)
    u, w = scaled([(0, ncrms)], 1)
    courant_equals_model(p, name, inp, u, w, "blocks (5, 6) and (0, 5)")
    run_equals_oracle(M, oracle, p, name, inp, u, w, "blocks (5, 6) and (0, 5), run")
    # a block of the Courant number after a block scale
    refill()
    scale(p, *SM.s_like(name, 2, 1, 9), 1, 9)
    u, w = scaled([(1, 9)], 2)
    courant_equals_model(p, name, inp, u, w, "block (1, 9), courant of (0, 3)", 0, 3)
    p.close()


# ---- 3. the array forms: u and w between bands, a stream of their own
@pytest.mark.parametrize("name", ["f64-array", "f32-array"])
def test_array_forms(mpdata, oracle, name):
    import torch
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    assert shape == (7, 5, 6)
    ncrms = shape[0]
    inp = SM.make(oracle, name)
    U, W = inp["u"], inp["w"]
    assert np.all(W[:, :, -1] != 0)
    su, sw = SM.s_like(name)
    wantu, wantw = SM.scale_uw(U, W, su, sw)

    def arrays():
        out = []
        for a in (U, W):
            raw, _, view = banded(a.T.shape, dt)
            view.copy_(to_dev(a))
            out.append((raw, raw.clone(), view))
        torch.cuda.synchronize()
        return out

    def bands_intact(b, what):
        assert torch.equal(b[0][:BAND], b[1][:BAND]) and torch.equal(b[0][-BAND:], b[1][-BAND:]), f"a band byte of {what} changed"

    bu, bw = arrays()
    fu, fw = dev_s(su), dev_s(sw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    M.scale_uw(bu[2], bw[2], fu[2], fw[2], stream=s)
    s.synchronize()
    assert_bitwise(to_host(bu[2]), wantu, f"{name}: u")
    assert_bitwise(to_host(bw[2]), wantw, f"{name}: w, level nz included")
    bands_intact(bu, "u")
    bands_intact(bw, "w")
    assert torch.equal(fu[0], fu[1]) and torch.equal(fw[0], fw[1]), "a byte of the factors or of their bands changed"
    # w = NULL: every byte of w is unchanged; u = NULL likewise (the current stream)
    bu, bw = arrays()
    M.scale_uw(bu[2], None, fu[2], None)
    torch.cuda.synchronize()
    assert_bitwise(to_host(bu[2]), wantu, f"{name}: u alone")
    assert torch.equal(bw[0], bw[1]), "a byte of w changed in a call without w"
    bands_intact(bu, "u")
    bu, bw = arrays()
    M.scale_uw(None, bw[2], None, fw[2])
    torch.cuda.synchronize()
    assert_bitwise(to_host(bw[2]), wantw, f"{name}: w alone")
    assert torch.equal(bu[0], bu[1]), "a byte of u changed in a call without u"
    bands_intact(bw, "w")
    # refused calls change nothing
    keepu, keepw = bu[0].clone(), bw[0].clone()
    L = M.lib()
    fn = L.mpdata_scale_uw_device if dt == np.float64 else L.mpdata_scale_uw_f32_device
    pu, pw, psu, psw = (ctypes.c_void_p(t.data_ptr()) for t in (bu[2], bw[2], fu[2], fw[2]))
    for args in ((None, None, None, None), (pu, pw, None, None), (pu, pw, psu, None), (pu, None, psu, psw), (None, pw, psu, psw),
                 (pu, pw, None, psw)):
        assert fn(ncrms, shape[1], shape[2], *args, None) == M.EINVAL, args
    for dims in ((0, 5, 6), (7, 0, 6), (7, 5, 1)):
        assert fn(*dims, pu, pw, psu, psw, None) == M.EINVAL, dims
    torch.cuda.synchronize()
    assert torch.equal(bu[0], keepu) and torch.equal(bw[0], keepw)


# ---- 4. the host forms equal the device form
@pytest.mark.parametrize("name,sw_", [("f64-blocks", {}), ("f32-blocks", dict(odd=True)), ("f32-nz12-ref", dict(ref=True)),
                                      ("f64-tall", dict(tall=True))], ids=lambda v: v if isinstance(v, str) else "")
def test_host_forms(mpdata, oracle, name, sw_):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = SM.make(oracle, name)
    a, b = new_plan(M, name, **sw_), new_plan(M, name, **sw_)
    m = model_of(oracle, name, inp)
    upload(a, inp)
    upload(b, inp)
    for k, (sl0, n, both) in enumerate(((ncrms - 1, 1, (True, True)), (1, ncrms - 2, (True, False)), (0, ncrms, (False, True)),
                                        (0, ncrms, (True, True)))):       # (the staging buffer grows)
        su, sw = SM.s_like(name, k, sl0, n)
        su, sw = (su if both[0] else None), (sw if both[1] else None)
        keep = [None if s is None else s.copy() for s in (su, sw)]
        b.scale_uw_host(su, sw, sl0, n)
        for s, c in zip((su, sw), keep):
            assert s is None or np.array_equal(LM.bits(s), LM.bits(c)), "the caller's factors"
        scale(a, su, sw, sl0, n)
        assert m.scale_uw(su, sw, sl0, n) is None
        ca, cb = cour(a, dt, nz - 1, 0, ncrms), cour(b, dt, nz - 1, 0, ncrms)
        want = CM.courant(m.a["u"], m.a["w"], inp["rho"], inp["adz"])
        for q, c in (("device form", ca), ("host form", cb)):
            assert_bitwise(c["clev"], want[0], f"{name} {q} {sl0, n}: clev")
            assert_bitwise(c["cinst"], want[1], f"{name} {q} {sl0, n}: cinst")
    a.run()
    b.run()
    assert m.run() is None
    same_as_model(M, a, name, m, "device form, run")
    same_as_model(M, b, name, m, "host form, run")
    # the form of the other precision; NULLs; nothing changed
    other = np.float32 if dt == np.float64 else np.float64
    s = np.ones((ncrms,), other)
    ps = ctypes.c_void_p(s.ctypes.data)
    L = M.lib()
    wrong, right = (L.mpdata_plan_scale_uw_f32, L.mpdata_plan_scale_uw) if dt == np.float64 else (L.mpdata_plan_scale_uw, L.mpdata_plan_scale_uw_f32)
    assert wrong(b._p, 0, ncrms, ps, ps) == M.ESTATE
    assert right(b._p, 0, ncrms, None, None) == M.EINVAL
    assert wrong(b._p, 0, ncrms, None, None) == M.EINVAL                      # (the NULLs before the state)
    assert wrong(b._p, 0, ncrms + 1, ps, ps) == M.EINVAL                      # (the range before both)
    same_as_model(M, b, name, m, "after the refused host calls")
    b.run()
    assert m.run() is None
    same_as_model(M, b, name, m, "after the refused host calls, run")
    a.close()
    b.close()


# ---- 5. errors: the code, and the plan's next run equals the model's
def test_errors(mpdata, oracle):
    import torch
    M = mpdata
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = SM.make(oracle, name)
    su, sw = SM.s_like(name)
    du, dw = to_dev(su), to_dev(sw)
    p = new_plan(M, name)
    m = SM.PlanModelScale(oracle, *shape, T, dt)
    L = M.lib()
    pu, pw = ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(dw.data_ptr())
    hu, hw = ctypes.c_void_p(su.ctypes.data), ctypes.c_void_p(sw.ctypes.data)
    # never filled: the state comes last
    assert _code(M, p.scale_uw, du, dw) == M.ESTATE == m.scale_uw(su, sw)
    assert _code(M, p.scale_uw_host, su, sw) == M.ESTATE
    assert L.mpdata_plan_scale_uw_device(p._p, 0, ncrms, None, None) == M.EINVAL == m.scale_uw(None, None)
    assert L.mpdata_plan_scale_uw_device(p._p, 0, ncrms + 1, pu, pw) == M.EINVAL == m.scale_uw(su, sw, 0, ncrms + 1)
    upload(p, inp)
    assert m.upload(inp) is None

    def run_and_compare(what):
        p.run()
        assert m.run() is None
        same_as_model(M, p, name, m, what)

    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, ncrms + 1), (ncrms, 1), (5, 7)):
        assert L.mpdata_plan_scale_uw_device(p._p, sl0, n, pu, pw) == M.EINVAL == m.scale_uw(su[:max(n, 1)], sw[:max(n, 1)], sl0, n), (sl0, n)
        assert L.mpdata_plan_scale_uw(p._p, sl0, n, hu, hw) == M.EINVAL, (sl0, n)
    run_and_compare("after the refused ranges, run")
    assert L.mpdata_plan_scale_uw_device(p._p, 0, ncrms, None, None) == M.EINVAL == m.scale_uw(None, None)
    assert b"both NULL" in L.mpdata_last_error()
    assert L.mpdata_plan_scale_uw(p._p, 0, ncrms, None, None) == M.EINVAL
    assert L.mpdata_plan_scale_uw_device(None, 0, ncrms, pu, pw) == M.EINVAL
    assert L.mpdata_plan_scale_uw(None, 0, ncrms, hu, hw) == M.EINVAL
    assert L.mpdata_plan_scale_uw_f32(p._p, 0, ncrms, hu, hw) == M.ESTATE        # the form of the other precision
    run_and_compare("after the refused NULLs and the other precision, run")
    # the plan does not hold the array being scaled: only the arrays asked for are tested
    ou, ow = SM.other(oracle, name)
    p.run_uw(to_dev(ou), to_dev(ow))
    assert m.run_uw(ou, ow) is None
    assert _code(M, p.scale_uw, du, dw) == M.ESTATE == m.scale_uw(su, sw)
    assert b"does not hold u" in L.mpdata_last_error()
    assert _code(M, p.scale_uw_host, su, None) == M.ESTATE == m.scale_uw(su, None)
    p.import_device(u=to_dev(ou))
    assert m.import_device({"u": ou}) is None
    assert _code(M, p.scale_uw, du, dw) == M.ESTATE == m.scale_uw(su, sw)
    assert b"does not hold w" in L.mpdata_last_error()
    assert _code(M, p.scale_uw, None, dw) == M.ESTATE == m.scale_uw(None, sw)
    p.scale_uw(du, None)                                                         # u alone is held, and asked for alone
    assert m.scale_uw(su, None) is None
    p.import_device(w=to_dev(ow))
    assert m.import_device({"w": ow}) is None
    p.scale_uw(None, dw)
    assert m.scale_uw(None, sw) is None
    run_and_compare("after run_uw, the refused calls and the imports, run")
    p.sync()
    assert torch.equal(du, to_dev(su)) and torch.equal(dw, to_dev(sw))
    p.close()


def test_multi_gpu_handle_and_shard_plan(mpdata, oracle, monkeypatch):
    M = mpdata
    monkeypatch.delenv("MPDATA_MULTI_XFER", raising=False)
    name = "f64-blocks"
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms = shape[0]
    inp = SM.make(oracle, name)
    su, sw = SM.s_like(name)
    p = new_plan(M, name, devices=[0, 0])
    upload(p, inp)
    m = model_of(oracle, name, inp)
    m.multi = True
    assert _code(M, p.scale_uw, to_dev(su), to_dev(sw)) == M.EUNSUPPORTED == m.scale_uw(su, sw)
    assert b"mpdata_plan_shard_plan" in M.lib().mpdata_last_error()
    assert _code(M, p.scale_uw_host, su, sw) == M.EUNSUPPORTED
    m.multi = False
    for g, (_, s0, nloc) in enumerate(p.shards()):
        q = p.shard_plan(g)
        a, b = np.ascontiguousarray(su[s0:s0 + nloc]), np.ascontiguousarray(sw[s0:s0 + nloc])
        scale(q, a, b)
        assert m.scale_uw(a, b, s0, nloc) is None
        q.close()
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "after the shard plans' scalings and a run")
    p.close()


# ---- 6. no state change; a factor of 1 keeps every bit
@pytest.mark.parametrize("name,sw_", [("f64-blocks", {}), ("f32-tall-blocks", dict(tall=True, odd=True))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_no_state_change(mpdata, oracle, name, sw_):
    M = mpdata
    shape, T, dt, _ = LM.INPUTS[name]
    ncrms, nx, nz = shape
    inp = SM.make(oracle, name)
    p = new_plan(M, name, **sw_)
    upload(p, inp)
    m = model_of(oracle, name, inp)
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # no run yet
    ones = np.ones(ncrms, dt)
    scale(p, ones, ones)
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # ... and the scaling is none
    courant_equals_model(p, name, inp, inp["u"], inp["w"], "factors of 1")
    p.set_boundary(M.BOUNDARY_PERIODIC)
    assert m.set_boundary(PM.PERIODIC) is None
    p.run()
    assert m.run() is None
    p.sync()
    ms = p.last_kernel_ms()
    su, sw = SM.s_like(name, 0, 3, 5)
    scale(p, su, sw, 3, 5)
    assert m.scale_uw(su, sw, 3, 5) is None
    assert p.last_kernel_ms() == ms and p.boundary == M.BOUNDARY_PERIODIC
    same_as_model(M, p, name, m, "f, flux after a scaling")   # (f and flux keep every bit; the halos were stale)
    p.set_timing(0)
    scale(p, ones, None)
    assert _code(M, p.last_kernel_ms) == M.ESTATE           # the timing pair stays off
    p.set_timing(1)
    p.run()
    assert m.run() is None
    same_as_model(M, p, name, m, "run after the scalings")
    p.close()
