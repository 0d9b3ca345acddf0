#!/usr/bin/env python3
"""Cost of periodic lateral boundaries (include/mpdata_hip.h 3a) at ncrms=65536 nx=32 nz=28 fp64, cold:
every step runs on a plan (field set) of its own, as bench.py does.  Per-step time (torch events around
the whole loop, after a warm-up) of
  given      : K runs of BOUNDARY_GIVEN plans                                   (FAST and EXACT)
  periodic   : K runs of BOUNDARY_PERIODIC plans: halo kernel + plain kernel   (FAST and EXACT)
  T=25       : one run of 25 tracers, GIVEN vs PERIODIC                         (FAST)
  run_uw     : mpdata_plan_run_uw with fresh wrapped u, w, GIVEN vs PERIODIC   (FAST)
  workaround : export_device + periodic_halo + import_device + run on a GIVEN plan (what a caller
               had to do per step before the boundary mode existed)               (FAST)
Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/periodic_bench.py [--steps K] [--sets N] [--json PATH] [--no-t25]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--sets", type=int, default=8)
ap.add_argument("--ncrms", type=int, default=65536)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=28)
ap.add_argument("--json", default=None)
ap.add_argument("--no-t25", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
ncrms, nx, nz = a.ncrms, a.nx, a.nz
sh = M.shapes(ncrms, nx, nz, 1)
ab1 = M.algorithmic_bytes(ncrms, nx, nz, 1)
out = {"shape": [ncrms, nx, nz], "steps": a.steps, "sets": a.sets}


def timed(fn, steps, warm):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def report(name, ms, ab=ab1):
    out[name] = ms
    print(f"{name:28s}: {ms:.4f} ms/step  frac {ab / ms / 1e6 / 8000:.4f}", flush=True)


small = {k: torch.empty(sh[k], dtype=torch.float64, device=dev) for k in ("rho", "rhow", "adz", "flux")}
for k in small:
    M.fill_synthetic(small[k], k, 100, 1)
ftmp = torch.empty(sh["f"], dtype=torch.float64, device=dev)
uws = []
for s in range(a.sets):
    u = M.empty_staggered(sh["u"], "u", torch.float64, dev)
    w = M.empty_staggered(sh["w"], "w", torch.float64, dev)
    M.fill_synthetic(u, "u", 100 + 31 * s, 1)
    M.fill_synthetic(w, "w", 100 + 31 * s, 1)
    M.periodic_halo(u=u, w=w)
    uws.append((u, w))


def make_plans(variant, T=1, n=None):
    M.set_variant(variant)
    plans = []
    for s in range(a.sets if n is None else n):
        p = M.Plan(ncrms, nx, nz, T)
        p.set_stream()
        p.set_timing(False)
        u, w = uws[s % a.sets]
        p.import_device(None, u, w, small["rho"], small["rhow"], small["adz"], None)
        for t in range(T):
            M.fill_synthetic(ftmp, "f", 100 + s * T + t, 1)
            p.import_device(ftmp, flux=small["flux"], first_tracer=t)
        plans.append(p)
    torch.cuda.synchronize()
    return plans


def boundary(plans, mode):
    for p in plans:
        p.set_boundary(mode)


K = a.steps
for vname, v in (("fast", M.VARIANT_FAST), ("exact", M.VARIANT_EXACT)):
    plans = make_plans(v)
    n = len(plans)
    report(f"given_{vname}", timed(lambda i: plans[i % n].run(), K, K))
    boundary(plans, M.BOUNDARY_PERIODIC)
    report(f"periodic_{vname}", timed(lambda i: plans[i % n].run(), K, K))
    if v == M.VARIANT_FAST:
        boundary(plans, M.BOUNDARY_GIVEN)
        report("run_uw_given_fast", timed(lambda i: plans[i % n].run_uw(*uws[(i + 1) % n]), K, K))
        boundary(plans, M.BOUNDARY_PERIODIC)
        report("run_uw_periodic_fast", timed(lambda i: plans[i % n].run_uw(*uws[(i + 1) % n]), K, K))
        boundary(plans, M.BOUNDARY_GIVEN)
        fx = [torch.empty(sh["f"], dtype=torch.float64, device=dev) for _ in range(2)]
        for p, (u, w) in zip(plans, uws):   # (run_uw leaves no velocities behind)
            p.import_device(None, u, w)
        torch.cuda.synchronize()
        cur = torch.cuda.current_stream()

        def workaround(i):
            p, f = plans[i % n], fx[i % 2]
            p.export_device(f=f)
            M.periodic_halo(f=f, stream=cur)
            p.import_device(f=f)
            p.run()
        report("workaround_fast", timed(workaround, K, K))
    for p in plans:
        p.close()
    del plans
    torch.cuda.empty_cache()

if not a.no_t25:
    T = 25
    abT = M.algorithmic_bytes(ncrms, nx, nz, T)
    plans = make_plans(M.VARIANT_FAST, T, n=2)
    report("t25_given_fast", timed(lambda i: plans[i % 2].run(), 4, 2), abT)
    boundary(plans, M.BOUNDARY_PERIODIC)
    report("t25_periodic_fast", timed(lambda i: plans[i % 2].run(), 4, 2), abT)
    for p in plans:
        p.close()

for key in ("fast", "exact"):
    out[f"ratio_periodic_{key}"] = out[f"periodic_{key}"] / out[f"given_{key}"]
out["ratio_run_uw"] = out["run_uw_periodic_fast"] / out["run_uw_given_fast"]
out["ratio_workaround"] = out["workaround_fast"] / out["given_fast"]
if "t25_given_fast" in out:
    out["ratio_t25"] = out["t25_periodic_fast"] / out["t25_given_fast"]
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
