"""The single-precision Fortran driver on an odd ncrms above 32 levels (include/mpdata_hip.h section 3f): with
MPDATA_F32_ODD_NCRMS=1 in its environment the drop-in call and the fp32 plan run on the packed kernels and match the fp32
oracle; without it the same command is the error it has always been."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE_SP = os.path.join(ROOT, "codesign-kernels_amd", "fortran", "advect_sp")


def drive(shape, dist, variant, dump, switch):
    env = {k: v for k, v in os.environ.items() if k != "MPDATA_F32_ODD_NCRMS"}
    if switch:
        env["MPDATA_F32_ODD_NCRMS"] = "1"
    return subprocess.run([EXE_SP, *map(str, shape), str(dist), str(variant), str(dump)], capture_output=True, text=True,
                          timeout=300, env=env)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dist,variant", [((101, 32, 58), 1, 0), ((101, 32, 58), 3, 0), ((101, 32, 58), 1, 1),
                                                ((33, 16, 72), 1, 0)])
def test_single_precision_driver_odd_ncrms(oracle, tmp_path, shape, dist, variant):
    assert os.path.exists(EXE_SP), "single-precision Fortran driver not built"
    ncrms, nx, nz = shape
    dump = tmp_path / "out.bin"
    res = drive(shape, dist, variant, dump, True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "HIP Timing:" in res.stdout
    inp = oracle.make_inputs(ncrms, nx, nz, seed=100, dist=dist, dtype=np.float32)
    f_ref, flux_ref = oracle.advect(inp)
    raw = np.fromfile(dump, dtype=np.float32)
    f = raw[:f_ref.size].reshape(f_ref.shape, order="F")
    flux = raw[f_ref.size:].reshape(flux_ref.shape, order="F")
    nzm = nz - 1
    if variant == 0:
        assert np.array_equal(f, f_ref)
        assert np.array_equal(flux, flux_ref)
    else:
        assert np.abs(f.astype(np.float64) - f_ref).max() < 1e-5
        d = np.abs(flux[:, :nzm].astype(np.float64) - flux_ref[:, :nzm])
        assert np.all(d <= 2e-5 * np.maximum(1.0, np.abs(flux_ref[:, :nzm])))
    assert np.array_equal(flux[:, nzm], inp["flux"][:, nzm])


@pytest.mark.gpu
def test_single_precision_driver_odd_ncrms_needs_the_switch(tmp_path):
    assert os.path.exists(EXE_SP), "single-precision Fortran driver not built"
    res = drive((101, 32, 58), 1, 0, tmp_path / "out.bin", False)
    assert res.returncode != 0, res.stdout
