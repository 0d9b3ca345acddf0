"""bench.py without --full: the headline and nothing else, and --dump-outputs holds what its last timed step computed
(EXACT variant: bit-identical to the CPU oracle on the same field set)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench_contract as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_its_last_step(oracle, tmp_path):
    n, nx, nz, ntr, steps = 8192, 32, 28, 3, 3
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--prewarm-ms", "20", "--prewarm-min-ms", "5", "--ncrms-per-gpu", str(n), "--tracers", str(ntr),
           "--variant", "exact", "--dump-outputs", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    C.check_headline(d, n, ntracers=ntr)
    assert d["steps"] == steps and d["unit"] == "cell-updates/s"
    assert d["roofline"]["kernel_ms_avg"] <= d["ms_per_step"] * 1.001
    for k in ("cpu_baseline", "layout_conversion", "tracer_batched", "reference_layout_device_call", "fp32",
              "exact_variant", "biharmonic_wk", "high_order_flux", "end_to_end_host_call"):
        assert k not in d, k
    assert "kernel_ms_samples" not in d["roofline"] and "measured_copy_GBs" not in d["roofline"]

    # the dump: the field set of the last timed step (3 timed sets + 1 scratch set: step 2 ran on set 2, once),
    # a seeded sample of the instances (3 tracers of 8192 instances are more than the dump's budget)
    import bench
    f, flux = np.load(out / "f.npy"), np.load(out / "flux.npy")
    per_instance = ntr * ((nz - 1) * (nx + 6) + nz) * 8
    k = min(n, bench.DUMP_BYTES // per_instance)
    assert k < n
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, k, replace=False))
    assert f.dtype == np.float64 and f.shape == (ntr, nz - 1, nx + 6, k) and flux.shape == (ntr, nz, k)
    s = steps - 1
    sh = oracle.shapes(n, nx, nz)
    inp = {key: oracle.fill_array(key, sh[key], 100 + 7919 * (s + 1), oracle.DIST_CONDITIONED)
           for key in ("u", "w", "rho", "rhow", "adz")}
    inp["flux"] = oracle.fill_array("flux", sh["flux"], 100, oracle.DIST_CONDITIONED)
    for t in range(ntr):
        inp["f"] = oracle.fill_array("f", sh["f"], 100 + s * ntr + t, oracle.DIST_CONDITIONED)
        f_ref, flux_ref = oracle.advect(inp)
        assert np.array_equal(f[t], f_ref[idx].T), t
        assert np.array_equal(flux[t], flux_ref[idx].T), t
