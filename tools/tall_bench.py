#!/usr/bin/env python3
"""Tall columns (include/mpdata_hip.h 3e): ms per step of one plan run at ncrms=4096 nx=32 nz=300 fp64,
one tracer, FAST and EXACT, cold: every launch runs on a plan (field set) of its own, as bench.py does.  One mode and
one library per invocation (raw ctypes on the few entry points every build of the library has, so that the SAME code
times another build -- the parent commit's, say -- given with --lib):
  --mode ref       the switch off: a reference-layout plan on the k-marching kernel
  --mode windowed  the switch on:  first run after an import of f (seams fresh: no refresh) and run after run
                   (the seam refresh inside the run's event pair)
  --mode inner     for comparison: an ordinary plan of ncrms * W instances of nz_w levels (what the windows are)
  --mode trace     windowed, a few runs after runs and nothing else: for `rocprofv3 --kernel-trace --stats -- python
                   tools/tall_bench.py --mode trace`, which gives the refresh kernel (window_seams_kernel) alone
Protocol: wake-up by plateau rule (groups of 8 launches, a host clock around each group and its synchronise, until
three consecutive groups agree within 1 %, at least 40 ms, at most --cap-ms), then --steps launches with the plan's own event pair around each
(mpdata_plan_last_kernel_ms); median, min and the samples are printed as one JSON line per variant.
usage: python tools/tall_bench.py --mode ref|windowed|inner|trace [--lib PATH] [--sets N] [--steps K] [--json PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["ref", "windowed", "inner", "trace"])
ap.add_argument("--lib", default=os.path.join(ROOT, "codesign-kernels_amd", "libmpdata_hip.so"))
ap.add_argument("--ncrms", type=int, default=4096)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=300)
ap.add_argument("--sets", type=int, default=8)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--cap-ms", type=float, default=1500.0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

import torch

assert torch.cuda.is_available(), "tall_bench.py measures on a GPU; there is none"
L = ctypes.CDLL(a.lib)
vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
L.mpdata_last_error.restype = ctypes.c_char_p
L.mpdata_plan_create.argtypes = [i64, ci, ci, ci, ctypes.POINTER(vp)]
L.mpdata_plan_import_device.argtypes = [vp] * 8 + [ci, ci]
L.mpdata_plan_run.argtypes = [vp]
L.mpdata_plan_sync.argtypes = [vp]
L.mpdata_plan_destroy.argtypes = [vp]
L.mpdata_plan_layout.argtypes = [vp]
L.mpdata_plan_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
L.mpdata_fill_synthetic_device.argtypes = [vp, ci, i64, i64, i64, i64, ctypes.c_uint64, ci, vp]
L.mpdata_algorithmic_bytes.restype = i64
L.mpdata_algorithmic_bytes.argtypes = [i64, ci, ci, ci]
SID = {"adz": 0, "f": 1, "u": 2, "w": 3, "rho": 4, "rhow": 5, "flux": 6}


def ck(rc):
    if rc != 0:
        raise RuntimeError(f"libmpdata_hip error {rc}: {L.mpdata_last_error().decode()}")


ncrms, nx, nz = a.ncrms, a.nx, a.nz
W = 1
if a.mode != "ref":
    L.mpdata_level_window.argtypes = [ci, ci] + [ctypes.POINTER(ci)] * 4
    k0, nzw = ci(), ci()
    W = L.mpdata_level_window(nz, 0, ctypes.byref(k0), ctypes.byref(nzw), None, None)
    if a.mode == "inner":
        ncrms, nz = ncrms * W, nzw.value
    else:
        L.mpdata_set_tall_columns(1)
        L.mpdata_plan_level_windows.argtypes = [vp]
nzm = nz - 1
shapes = {"adz": (nzm, ncrms), "f": (nzm, nx + 6, ncrms), "u": (nzm, nx + 5, ncrms), "w": (nz, nx + 4, ncrms),
          "rho": (nzm, ncrms), "rhow": (nz, ncrms), "flux": (nz, ncrms)}
dev = torch.device("cuda", 0)
src = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in shapes.items()}


def fill(k, seed):
    t = src[k]
    ck(L.mpdata_fill_synthetic_device(t.data_ptr(), SID[k], t.numel() // ncrms, ncrms, 0, ncrms, seed, 1, None))


def ptr(k):
    return ctypes.c_void_p(src[k].data_ptr())


def import_f(p, seed):
    fill("f", seed)
    torch.cuda.synchronize()
    ck(L.mpdata_plan_import_device(p, ptr("f"), None, None, None, None, None, None, 0, 1))
    ck(L.mpdata_plan_sync(p))


def make_plans():
    plans = []
    for s in range(a.sets):
        p = vp()
        ck(L.mpdata_plan_create(ncrms, nx, nz, 1, ctypes.byref(p)))
        for k in src:
            fill(k, 100 + 31 * s)
        torch.cuda.synchronize()
        ck(L.mpdata_plan_import_device(p, *[ptr(k) for k in ("f", "u", "w", "rho", "rhow", "adz", "flux")], 0, 1))
        ck(L.mpdata_plan_sync(p))
        plans.append(p)
    return plans


def run_ms(p):
    ck(L.mpdata_plan_run(p))
    ms = ctypes.c_double()
    ck(L.mpdata_plan_last_kernel_ms(p, ctypes.byref(ms)))
    return ms.value


def wake_up(plans):
    """plateau rule of bench.py on this mode's own launches"""
    t0, groups, n = time.perf_counter(), [], 0
    while True:
        t1 = time.perf_counter()
        for _ in range(8):
            ck(L.mpdata_plan_run(plans[n % len(plans)]))
            n += 1
        for p in plans:
            ck(L.mpdata_plan_sync(p))
        groups.append((time.perf_counter() - t1) * 1e3 / 8)
        used = (time.perf_counter() - t0) * 1e3
        last = groups[-3:]
        if len(last) == 3 and used >= 40 and max(last) - min(last) <= 0.01 * min(last):
            return {"plateau_reached": True, "groups": len(groups), "ms_used": used}
        if used >= a.cap_ms:
            return {"plateau_reached": False, "groups": len(groups), "ms_used": used}


def stats(name, samples, out, ab):
    med = statistics.median(samples)
    out[name] = {"ms_median": med, "ms_min": min(samples), "ms_samples": [round(x, 5) for x in samples],
                 "frac_of_8TBs_median": ab / med / 1e6 / 8000}
    print(f"{name:34s}: median {med:.4f} ms  min {min(samples):.4f} ms  frac {ab / med / 1e6 / 8000:.4f}", flush=True)


out = {"mode": a.mode, "lib": os.path.relpath(a.lib, ROOT), "shape": [ncrms, nx, nz], "windows": W, "sets": a.sets, "steps": a.steps}
# the bytes the TALL problem needs, whatever the mode moves
ab = L.mpdata_algorithmic_bytes(a.ncrms, a.nx, a.nz, 1)
for vname, v in (("fast", 1), ("exact", 0)):
    L.mpdata_set_variant(v)
    plans = make_plans()
    lay = L.mpdata_plan_layout(plans[0])
    out[f"layout_{vname}"] = lay
    if a.mode in ("windowed", "trace"):
        assert L.mpdata_plan_level_windows(plans[0]) == W and lay == 1
    if a.mode == "ref":
        assert lay == 0
    if a.mode == "trace":
        for i in range(2 * a.sets):
            ck(L.mpdata_plan_run(plans[i % a.sets]))
        for p in plans:
            ck(L.mpdata_plan_sync(p))
    else:
        out[f"wake_up_{vname}"] = wake_up(plans)
        if a.mode == "windowed":
            first = []
            for i in range(a.steps):
                p = plans[i % a.sets]
                import_f(p, 1000 + i)     # (untimed: the seams are fresh afterwards)
                first.append(run_ms(p))
            stats(f"first_run_{vname}", first, out, ab)
            for p in plans:                # every plan has run since its import: the next run refreshes
                ck(L.mpdata_plan_sync(p))
        stats(("run_after_run_" if a.mode == "windowed" else "run_") + vname, [run_ms(plans[i % a.sets]) for i in range(a.steps)], out, ab)
    for p in plans:
        ck(L.mpdata_plan_destroy(p))
    torch.cuda.synchronize()
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
