#!/usr/bin/env python3
"""fp32 with an odd ncrms on the packed kernels (include/mpdata_hip.h 3f): what the phantom half costs.
One mode, one shape and one library per invocation (raw ctypes on entry points every build of the library has, so that
the SAME code times another build -- the parent commit's, say -- given with --lib; a library without
mpdata_set_f32_odd_ncrms simply keeps its behaviour), fp32, one tracer, FAST and EXACT, cold: every launch works on a
plan (field set) of its own, as bench.py does.
  --mode run      ms of one plan run by the plan's own event pair (mpdata_plan_last_kernel_ms).  --switch 0 at an odd
                  ncrms and nz <= 32 is the path without the feature: a reference-layout plan on the
                  one-instance-per-lane kernel
  --mode convert  whole-plan import (f; u + w) and export (f; f + flux) between reference-layout device arrays and the
                  plan, ms by an event pair on the plan's stream
  --mode call     the device call mpdata_advect_scalar2d_f32_device (above 64 levels, or above 32 with an odd ncrms: import +
                  run + export through the thread's staged plan), ms by an event pair on the stream
Protocol: wake-up by plateau rule (groups of 8 launches, a host clock around each group and its synchronise, until three
consecutive groups agree within 1 %, at least 40 ms, at most --cap-ms), then --steps timed launches; median, min and
the samples are printed as one JSON line.  Interleave invocations to compare (docs/EXPERIMENTS.md H).
usage: python tools/odd_ncrms_bench.py --mode run|convert|call --ncrms N [--nz 58] [--switch 0|1] [--lib PATH] [--json PATH]"""
import argparse
import ctypes
import json
import os
import statistics
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--mode", required=True, choices=["run", "convert", "call"])
ap.add_argument("--lib", default=os.path.join(ROOT, "codesign-kernels_amd", "libmpdata_hip.so"))
ap.add_argument("--ncrms", type=int, required=True)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=58)
ap.add_argument("--switch", type=int, default=1, choices=[0, 1])
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--cap-ms", type=float, default=1500.0)
ap.add_argument("--json", default=None)
a = ap.parse_args()

import torch

assert torch.cuda.is_available(), "odd_ncrms_bench.py measures on a GPU; there is none"
L = ctypes.CDLL(a.lib)
vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
L.mpdata_last_error.restype = ctypes.c_char_p
L.mpdata_plan_create_f32.argtypes = [i64, ci, ci, ci, ctypes.POINTER(vp)]
L.mpdata_plan_import_device.argtypes = [vp] * 8 + [ci, ci]
L.mpdata_plan_export_device.argtypes = [vp] * 3 + [ci, ci]
L.mpdata_plan_set_stream.argtypes = [vp, vp]
L.mpdata_plan_run.argtypes = [vp]
L.mpdata_plan_sync.argtypes = [vp]
L.mpdata_plan_destroy.argtypes = [vp]
L.mpdata_plan_layout.argtypes = [vp]
L.mpdata_plan_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
L.mpdata_fill_synthetic_f32_device.argtypes = [vp, ci, i64, i64, i64, i64, ctypes.c_uint64, ci, vp]
L.mpdata_advect_scalar2d_f32_device.argtypes = [i64, ci, ci, ci] + [vp] * 8
SID = {"adz": 0, "f": 1, "u": 2, "w": 3, "rho": 4, "rhow": 5, "flux": 6}
ORDER = ("f", "u", "w", "rho", "rhow", "adz", "flux")
has_switch = hasattr(L, "mpdata_set_f32_odd_ncrms")
if has_switch:
    L.mpdata_set_f32_odd_ncrms(a.switch)


def ck(rc):
    if rc != 0:
        raise RuntimeError(f"libmpdata_hip error {rc}: {L.mpdata_last_error().decode()}")


ncrms, nx, nz = a.ncrms, a.nx, a.nz
nzm = nz - 1
shapes = {"adz": (nzm, ncrms), "f": (nzm, nx + 6, ncrms), "u": (nzm, nx + 5, ncrms), "w": (nz, nx + 4, ncrms),
          "rho": (nzm, ncrms), "rhow": (nz, ncrms), "flux": (nz, ncrms)}
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
sh = ctypes.c_void_p(stream.cuda_stream)


def field_set(seed):
    s = {k: torch.empty(v, dtype=torch.float32, device=dev) for k, v in shapes.items()}
    for k, t in s.items():
        ck(L.mpdata_fill_synthetic_f32_device(t.data_ptr(), SID[k], t.numel() // ncrms, ncrms, 0, ncrms, seed, 1, None))
    torch.cuda.synchronize()
    return s


def ptrs(s, keys=ORDER):
    return [ctypes.c_void_p(s[k].data_ptr()) if k in keys else None for k in ORDER]


def wake_up(launch, sync):
    t0, groups, n = time.perf_counter(), [], 0
    while True:
        t1 = time.perf_counter()
        for _ in range(8):
            launch(n)
            n += 1
        sync()
        groups.append((time.perf_counter() - t1) * 1e3 / 8)
        used = (time.perf_counter() - t0) * 1e3
        last = groups[-3:]
        if len(last) == 3 and used >= 40 and max(last) - min(last) <= 0.01 * min(last):
            return {"plateau_reached": True, "groups": len(groups), "ms_used": used}
        if used >= a.cap_ms:
            return {"plateau_reached": False, "groups": len(groups), "ms_used": used}


def evtimed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


out = {"mode": a.mode, "lib": os.path.relpath(a.lib, ROOT), "shape": [ncrms, nx, nz], "switch": a.switch if has_switch else None,
       "sets": a.sets, "steps": a.steps}


def stats(name, samples):
    med = statistics.median(samples)
    out[name] = {"ms_median": med, "ms_min": min(samples), "ms_samples": [round(x, 5) for x in samples]}
    print(f"{name:28s}: median {med:.4f} ms  min {min(samples):.4f} ms", flush=True)


for vname, v in (("fast", 1), ("exact", 0)):
    L.mpdata_set_variant(v)
    sets = [field_set(100 + 31 * s) for s in range(a.sets)]
    if a.mode == "call":
        def call(i):
            ck(L.mpdata_advect_scalar2d_f32_device(ncrms, nx, nz, 1, *ptrs(sets[i % a.sets]), sh))
        out[f"wake_up_{vname}"] = wake_up(call, torch.cuda.synchronize)
        stats(f"call_{vname}", [evtimed(lambda: call(i)) for i in range(a.steps)])
        ck(L.mpdata_release_host_buffers())
        continue
    plans = []
    for s in sets:
        p = vp()
        ck(L.mpdata_plan_create_f32(ncrms, nx, nz, 1, ctypes.byref(p)))
        if a.mode == "convert":
            ck(L.mpdata_plan_set_stream(p, sh))
        ck(L.mpdata_plan_import_device(p, *ptrs(s), 0, 1))
        ck(L.mpdata_plan_sync(p))
        plans.append(p)
    out[f"layout_{vname}"] = L.mpdata_plan_layout(plans[0])

    def sync_all():
        for p in plans:
            ck(L.mpdata_plan_sync(p))
    out[f"wake_up_{vname}"] = wake_up(lambda i: ck(L.mpdata_plan_run(plans[i % a.sets])), sync_all)
    if a.mode == "run":
        ms = ctypes.c_double()
        samples = []
        for i in range(a.steps):
            ck(L.mpdata_plan_run(plans[i % a.sets]))
            ck(L.mpdata_plan_last_kernel_ms(plans[i % a.sets], ctypes.byref(ms)))
            samples.append(ms.value)
        stats(f"run_{vname}", samples)
    else:
        def imp(i, keys):
            ck(L.mpdata_plan_import_device(plans[i % a.sets], *ptrs(sets[i % a.sets], keys), 0, 1))

        def exp(i, flux):
            s = sets[i % a.sets]
            ck(L.mpdata_plan_export_device(plans[i % a.sets], s["f"].data_ptr(), s["flux"].data_ptr() if flux else None, 0, 1))
        for name, fn in (("import_f", lambda i: imp(i, ("f",))), ("import_uw", lambda i: imp(i, ("u", "w"))),
                         ("export_f", lambda i: exp(i, False)), ("export_f_flux", lambda i: exp(i, True))):
            stats(f"{name}_{vname}", [evtimed(lambda: fn(i)) for i in range(a.steps)])
    for p in plans:
        ck(L.mpdata_plan_destroy(p))
    del sets
    torch.cuda.synchronize()
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
