"""Multi-GPU plans on DIFFERENT physical devices -- the tests that light up on a box with two or more GPUs
(they skip on a one-GPU box, where tests/test_multi_plan.py maps every rank to device 0 and
tests/test_multi_fake_rccl.py runs the RCCL branch against a stand-in).

What replaces the reference's `!$acc update device(...)` / `update host(...)` (reference :105-109, :241-242)
for a sharded run: scatter of the inputs, gather of f and flux.  Every case runs in a child
process (tests/stubs/run_multi_real_case.py): devices [0, 1] and -- with four or more -- all of them; transports
rccl | p2p | direct | the default for the data's origin; host-origin and root-GPU-origin arrays; mpdata_plan_run_uw
on the sharded plan; a full-size case generated on the root GPU.  Bitwise equal to a single-GPU plan and to the
oracle on sampled blocks; `ranks_seen == ngpus` on the RCCL transport.

The library's DEFAULT ordering of a transfer (per-array stream order + events, no host synchronisation between
the 5 + 2 ntracers arrays) has never run on xGMI.  When a case fails in that mode, the TEST runs it once more in
a fresh process under MPDATA_MULTI_SYNC=1 (the bring-up fallback: every stream synchronised after every array)
and the failure message says which mode passed; gpurun_out/multi_real_devices.json records every case either way.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = os.path.join(ROOT, "tests", "stubs", "run_multi_real_case.py")
RECORD = os.path.join(ROOT, "gpurun_out", "multi_real_devices.json")


def _ndev():
    try:
        import codesign_kernels_amd as M
        return M.device_count()
    except Exception:
        return 0


_HUNG = []   # a child that had to be killed at its timeout: the remaining real-device cases of this session are skipped
             # (a node on which transfers hang would otherwise hold the test run for timeout x cases x 2)


def _child(case, sync_each, timeout=300):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MPDATA_MULTI_SYNC", None)
    env.pop("MPDATA_MULTI_DEVICES", None)
    if sync_each:
        env["MPDATA_MULTI_SYNC"] = "1"
    try:
        r = subprocess.run([sys.executable, RUNNER, json.dumps(case)], env=env, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as exc:
        _HUNG.append(case)
        return {"ok": False, "error": f"timeout after {timeout} s (a hang)", "stderr": str(exc.stderr or "")[-1500:]}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        return {"ok": False, "error": f"rc {r.returncode}", "stderr": r.stderr[-2500:], "stdout": r.stdout[-500:]}
    return json.loads(lines[-1][len("RESULT "):])


def _record(case, entry):
    try:
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        allr = json.load(open(RECORD)) if os.path.exists(RECORD) else []
        allr.append({"case": case, **entry})
        json.dump(allr, open(RECORD, "w"), indent=1)
    except Exception:
        pass


def run_case(case):
    """default ordering first; on failure ONE retry in a fresh process with MPDATA_MULTI_SYNC=1.
    Returns the result of the mode that passed; fails the test with both reports otherwise -- and also when only
    the fallback passed (the default ordering is what ships)."""
    if _HUNG:
        pytest.skip("an earlier real-device case of this session hung (%s): not trying further ones" % json.dumps(_HUNG[0]))
    res = _child(case, False)
    if res.get("ok"):
        _record(case, {"mode_passed": "queued (default)", "result": res})
        return res
    res2 = _child(case, True) if len(_HUNG) < 2 else {"ok": False, "error": "not retried: two cases hung already"}
    _record(case, {"mode_passed": "MPDATA_MULTI_SYNC=1" if res2.get("ok") else None, "default": res, "sync": res2})
    if res2.get("ok"):
        pytest.fail("the DEFAULT (queued) ordering failed on real devices, MPDATA_MULTI_SYNC=1 passed: "
                    + json.dumps(res)[:3000])
    pytest.fail("failed in both orderings.  default: " + json.dumps(res)[:2000] + "\nsync: " + json.dumps(res2)[:2000])


def _device_sets():
    n = _ndev()
    sets = [[0, 1]] if n >= 2 else []
    if n >= 4:
        sets.append(list(range(n)))
        sets.append([n - 1, 0, 1])       # a root that is not device 0, an odd number of ranks
    return sets


needs2 = pytest.mark.skipif(_ndev() < 2, reason="needs two or more GPUs (skips on the one-GPU test box)")


@pytest.mark.gpu
def test_the_case_runner_itself_on_one_device():
    """the runner of this file on a box with ONE GPU: both ranks on device 0 (peer-copy transport), so that the
    harness the multi-GPU box will use has run before it gets there"""
    res = _child({"devices": [0, 0], "xfer": "default", "origin": "device", "shape": [131, 32, 28], "T": 2,
                  "run_uw": False}, False)
    assert res.get("ok"), res
    assert res["transport"] == "p2p" and res["ranks_seen"] == 0 and res["ngpus"] == 2
    res = _child({"devices": [0, 0], "xfer": "direct", "origin": "host", "shape": [70, 9, 12], "T": 1,
                  "run_uw": True}, True)
    assert res.get("ok") and res["sync_each"], res


@needs2
@pytest.mark.gpu
@pytest.mark.parametrize("xfer", ["default", "rccl", "p2p", "direct"])
@pytest.mark.parametrize("origin", ["host", "device"])
def test_sharded_plan_on_real_devices(xfer, origin):
    for devices in _device_sets():
        for shape, T in (([4099, 32, 28], 1), ([1000, 9, 12], 3)):
            if shape[0] < len(devices):
                continue
            res = run_case({"devices": devices, "xfer": xfer, "origin": origin, "shape": shape, "T": T, "run_uw": False})
            distinct = len(set(devices)) == len(devices)
            want = {"default": "direct" if origin == "host" else "rccl"}.get(xfer, xfer)
            assert res["transport"] == want, res
            assert res["ngpus"] == len(devices)
            if res["transport"] == "rccl" and distinct:
                assert res["ranks_seen"] == len(devices), res        # ncclCommCount of the plan's communicator


@needs2
@pytest.mark.gpu
@pytest.mark.parametrize("xfer", ["default", "p2p"])
def test_run_uw_on_a_sharded_plan_on_real_devices(xfer):
    for devices in _device_sets():
        res = run_case({"devices": devices, "xfer": xfer, "origin": "device", "shape": [2050, 32, 28], "T": 1,
                        "run_uw": True})
        assert res["ngpus"] == len(devices)


@needs2
@pytest.mark.gpu
def test_full_size_shards_generated_on_the_root_gpu():
    """BASELINE.json configs[2] per GPU (65536 instances each), two tracers, arrays generated on the root GPU and
    scattered over RCCL: the queue of 5 + 2 T arrays with 0.5-GB messages, FAST variant within 1e-12 of the oracle
    on sampled blocks and bitwise equal to the single-GPU plan."""
    for devices in _device_sets()[:2]:
        n = 65536 * len(devices) if len(devices) <= 2 else 32768 * len(devices)
        res = run_case({"devices": devices, "xfer": "default", "origin": "device", "shape": [n, 32, 28], "T": 2,
                        "run_uw": False, "big": True, "variant": 1})
        assert res["transport"] == "rccl" and res["ranks_seen"] == len(devices), res
        assert res["scatter_GBs_per_link"] > 0 and res["gather_GBs_per_link"] > 0


@needs2
@pytest.mark.gpu
@pytest.mark.parametrize("ntr,ngpus", [(1, 2), (3, 2), (2, 0)])
def test_fortran_driver_device_mode_on_real_devices(oracle, ntr, ngpus):
    """./advect ... ntracers ngpus device -- the Fortran driver's mode = device on ngpus DIFFERENT GPUs
    (ngpus = 0: all of them): global arrays generated on the root GPU, scattered over RCCL, advected, gathered,
    summed on the device; checksums against the oracle, `RCCL ranks seen` == ngpus."""
    import re
    exe = os.path.join(ROOT, "codesign-kernels_amd", "fortran", "advect")
    assert os.path.exists(exe), "Fortran driver not built"
    if _HUNG:
        pytest.skip("an earlier real-device case of this session hung")
    ngpus = ngpus or _ndev()
    ncrms, nx, nz, dist = 96 * ngpus + 1, 32, 28, 1
    inp = oracle.make_inputs(ncrms, nx, nz, seed=100, dist=dist, ntracers=ntr)
    f_ref, flux_ref = oracle.advect(inp, nthreads=4)
    out = None
    for sync_each in (False, True):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("MPDATA_MULTI_DEVICES", None)
        env.pop("MPDATA_MULTI_SYNC", None)
        if sync_each:
            env["MPDATA_MULTI_SYNC"] = "1"
        try:
            res = subprocess.run([exe, str(ncrms), str(nx), str(nz), str(dist), "0", "-", "-", str(ntr), str(ngpus),
                                  "device"], capture_output=True, text=True, timeout=300, env=env)
        except subprocess.TimeoutExpired:
            _HUNG.append({"fortran_driver": True, "ngpus": ngpus, "sync_each": sync_each})
            out = "timeout (a hang)"
            continue
        if res.returncode != 0:
            out = res.stdout + res.stderr
            continue
        out = res.stdout
        f = re.search(r"checksum f\s*:\s*([0-9.Ee+-]+)", out)
        x = re.search(r"checksum flux\s*:\s*([0-9.Ee+-]+)", out)
        ranks = re.search(r"RCCL ranks seen[^:]*:\s*(\d+)", out)
        good = f and x and ranks and int(ranks.group(1)) == ngpus and \
            float(f.group(1)) == pytest.approx(float(f_ref.sum()), rel=1e-12) and \
            float(x.group(1)) == pytest.approx(float(flux_ref[:, :nz - 1].sum()), rel=1e-10, abs=1e-9)
        if good:
            assert not sync_each, "the driver only passed under MPDATA_MULTI_SYNC=1:\n" + out
            assert "mode: device" in out and "scatter seconds" in out and "gather  seconds" in out
            return
    pytest.fail("Fortran driver, mode = device, ngpus = %d: failed in both orderings\n%s" % (ngpus, out))


@needs2
@pytest.mark.gpu
def test_bench_on_two_real_gpus_with_the_plain_command():
    """`python3 bench.py --gpus 2 ...` (no launcher, no rehearsal mode): two ranks over RCCL on two devices"""
    if _HUNG:
        pytest.skip("an earlier real-device case of this session hung")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MPDATA_BENCH_REHEARSAL"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "5", "--warmup", "2",
                          "--ncrms-per-gpu", "16384", "--batched-tracers", "3", "--batched-steps", "2", "--no-fp32",
                          "--no-bwk", "--no-x2", "--no-shared-block", "--no-exact", "--block-timeout", "120"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks_seen"] == 2 and sorted(d["config"]["devices_seen"]) == [0, 1]
    assert d["value"] > 0 and d["tracer_batched"]["value"] > 0
    sg = d["scatter_gather"]
    assert "error" not in sg and sg["scatter_GBs_per_link"] > 0 and sg["gather_GBs_per_link"] > 0
