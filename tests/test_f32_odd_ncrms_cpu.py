"""CPU tests of fp32 with an odd ncrms on the packed kernels (include/mpdata_hip.h section 3f).

The feature rests on one fact: no statement of the routine couples two CRM instances, so a problem of ncrms + 1
instances whose last instance repeats instance ncrms - 1 (the plan's phantom half) computes instances 0 .. ncrms-1 of
the odd problem bit for bit, and the two copies stay equal.  Checked here with the fp32 CPU oracle alone; the switch
itself needs no device either."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bitwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4, 3), (3, 8, 6), (7, 5, 33)]
REGIMES = ["conditioned", "raw_signed", "fronts"]


def make(oracle, shape, regime):
    if regime == "fronts":
        from oracle import regimes
        return regimes.make("fronts", *shape, seed=100, dtype=np.float32)
    dist = oracle.DIST_CONDITIONED if regime == "conditioned" else oracle.DIST_RAW_SIGNED
    return oracle.make_inputs(*shape, seed=100, dist=dist, dtype=np.float32)


def padded(inp):
    """the arrays of ncrms + 1 instances: the last one a copy of instance ncrms - 1"""
    return {k: np.asfortranarray(np.concatenate([v, v[-1:]], axis=0)) for k, v in inp.items()}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phantom_instance_changes_nothing(oracle, shape, regime):
    inp = make(oracle, shape, regime)
    n = shape[0]
    assert inp["f"].dtype == np.float32 and inp["f"].shape[0] == n and n % 2 == 1
    f_ref, flux_ref = oracle.advect(inp)
    f_pad, flux_pad = oracle.advect(padded(inp))
    assert f_pad.shape[0] == n + 1 and flux_pad.shape == (n + 1, shape[2])
    assert_bitwise(f_pad[:n], f_ref, "f of the first ncrms instances")
    assert_bitwise(flux_pad[:n], flux_ref, "flux of the first ncrms instances")
    assert_bitwise(f_pad[n], f_pad[n - 1], "f: phantom against the last instance")
    assert_bitwise(flux_pad[n], flux_pad[n - 1], "flux: phantom against the last instance")


def test_switch_round_trip(mpdata):
    M = mpdata
    prev = M.set_f32_odd_ncrms(0)
    try:
        assert M.set_f32_odd_ncrms(1) == 0
        assert M.set_f32_odd_ncrms(7) == 1      # not a setting: only queries
        assert M.set_f32_odd_ncrms(-1) == 1
        assert M.set_f32_odd_ncrms(0) == 1
        assert M.set_f32_odd_ncrms(0) == 0
    finally:
        M.set_f32_odd_ncrms(prev)


@pytest.mark.parametrize("env,want", [(None, 0), ("1", 1), ("0", 0)])
def test_switch_from_environment(env, want):
    """MPDATA_F32_ODD_NCRMS presets the switch: read in a child process, where nothing has touched the library yet"""
    e = {k: v for k, v in os.environ.items() if k != "MPDATA_F32_ODD_NCRMS"}
    if env is not None:
        e["MPDATA_F32_ODD_NCRMS"] = env
    code = "import codesign_kernels_amd as M; print(M.set_f32_odd_ncrms(-1))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout.strip().splitlines()[-1]) == want


@pytest.mark.parametrize("on", [0, 1])
def test_argument_errors_need_no_device(mpdata, on):
    """bad sizes and null pointers come back as MPDATA_EINVAL before any device call, with the switch on or off"""
    import ctypes
    M = mpdata
    L = M.lib()
    prev = M.set_f32_odd_ncrms(on)
    try:
        p = ctypes.c_void_p()
        for dims in ((0, 5, 33, 1), (3, 0, 33, 1), (3, 5, 2, 1), (3, 5, 33, 0)):
            assert L.mpdata_plan_create_f32(*dims, ctypes.byref(p)) == M.EINVAL and not p.value
        assert L.mpdata_plan_create_f32(3, 5, 33, 1, None) == M.EINVAL
        L.mpdata_advect_scalar2d_f32_device.restype = ctypes.c_int
        assert L.mpdata_advect_scalar2d_f32_device(ctypes.c_int64(3), 5, 33, 1, *[None] * 8) == M.EINVAL
        assert L.mpdata_advect_scalar2d_f32_device(ctypes.c_int64(0), 5, 33, 1, *[None] * 8) == M.EINVAL
    finally:
        M.set_f32_odd_ncrms(prev)
