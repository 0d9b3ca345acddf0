"""CPU tests of the level statistics (include/mpdata_hip.h 3g): the model on a hand-written case, the guard on the
seeded inputs of the GPU tests, the C-ABI's declarations and exports, and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import level_stats_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_level_stats_device", "mpdata_plan_level_stats", "mpdata_plan_level_stats_f32",
         "mpdata_level_stats_device", "mpdata_level_stats_f32_device")


def test_model_on_a_hand_written_case():
    """2 instances x 3 interior columns x 2 levels; the halo columns hold a value that would show in every result"""
    f = np.full((2, 9, 2), 1e30, order="F")
    f[0, 3:6, 0] = [1.0, 2.0, 4.0]
    f[1, 3:6, 0] = [1.0, 1e16, -1e16]     # order matters: (1 + 1e16) - 1e16 = 0, not 1
    f[0, 3:6, 1] = [-3.0, 5.0, 0.5]
    f[1, 3:6, 1] = [0.25, 0.25, 0.25]
    s, mn, mx = LM.level_stats(f)
    assert s.shape == mn.shape == mx.shape == (2, 2) and s.dtype == np.float64
    assert s.tolist() == [[7.0, 2.5], [0.0, 0.75]]
    assert mn.tolist() == [[1.0, -3.0], [-1e16, 0.25]]
    assert mx.tolist() == [[4.0, 5.0], [1e16, 0.25]]
    assert LM.sum_reversed(f)[1, 0] == 1.0 and LM.sum_pairwise(f)[1, 0] == 0.0   # (-1e16 + 1e16) + 1 = 1
    f32 = np.asfortranarray(f.astype(np.float32))
    assert LM.level_stats(f32)[0].dtype == np.float32
    # a sum that starts from +0.0 gives +0.0 on a column of -0.0
    z = np.full((1, 7, 1), -0.0, order="F")
    assert not np.signbit(LM.level_stats(z)[0][0, 0])


@pytest.mark.parametrize("name", [k for k, v in LM.INPUTS.items() if v[0][1] >= 3])
def test_inputs_can_expose_a_wrong_order(oracle, name):
    """In at least a quarter of the (sl, k[, t]) entries the defined sum differs in bit pattern from the reversed-order
    sum, and from a pairwise sum; and the inputs hold no -0.0 (the sign of a zero min / max is unspecified)."""
    shape, T, dt, seed = LM.INPUTS[name]
    f = LM.make(oracle, shape, T, dt, seed)["f"]
    assert f.dtype == dt and not LM.has_negative_zero(f) and np.all(np.isfinite(f))
    s = LM.level_stats(f)[0]
    rev = float(np.mean(LM.bits(s) != LM.bits(LM.sum_reversed(f))))
    pair = float(np.mean(LM.bits(s) != LM.bits(LM.sum_pairwise(f))))
    print(f"{name}: reversed differs in {rev:.2f}, pairwise in {pair:.2f} of {s.size} entries")
    assert rev >= 0.25 and pair >= 0.25, (name, rev, pair)


def test_header_declares_and_library_exports(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
        assert hasattr(mpdata.lib(), n), n
    assert "---- 3g." in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", mpdata.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_level_stats_device, L.mpdata_level_stats_f32_device):
        assert fn(4, 5, 6, 1, None, one, one, one, None) == mpdata.EINVAL          # null f
        assert b"null f" in L.mpdata_last_error()
        assert fn(4, 0, 6, 1, one, one, one, one, None) == mpdata.EINVAL           # nx < 1
        assert fn(4, 5, 1, 1, one, one, one, one, None) == mpdata.EINVAL           # nz < 2
        assert b"nz=1" in L.mpdata_last_error()
        assert fn(4, 5, 6, 1, one, None, None, None, None) == mpdata.EINVAL        # all outputs NULL
        assert fn(0, 5, 6, 1, one, one, one, one, None) == mpdata.EINVAL
        assert fn(4, 5, 6, 0, one, one, one, one, None) == mpdata.EINVAL
    assert L.mpdata_plan_level_stats_device(None, 0, 1, one, one, one, 0, 1) == mpdata.EINVAL
    assert L.mpdata_plan_level_stats(None, 0, 1, one, one, one) == mpdata.EINVAL
    assert L.mpdata_plan_level_stats_f32(None, 0, 1, one, one, one) == mpdata.EINVAL
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert L.mpdata_plan_level_stats_device(one, sl0, n, one, one, one, 0, 1) == mpdata.EINVAL


def test_new_kernels_do_not_spill():
    """the resource-usage report the build writes next to the object of mpdata_stats.hip"""
    rep = os.path.join(ROOT, "codesign-kernels_amd", "csrc", "mpdata_stats.usage.txt")
    if not os.path.exists(rep):
        pytest.skip("no resource-usage report (library not built here)")
    txt = open(rep).read()
    assert len(re.findall(r"Function Name: \S*level_stats_kernel", txt)) == 4
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)] == [0, 0, 0, 0]
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
