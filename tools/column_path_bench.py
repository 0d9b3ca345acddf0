#!/usr/bin/env python3
"""Time of the mass-weighted column integrals of a resident plan (include/mpdata_hip.h 3k) at ncrms=65536 nx=32 nz=28,
fp64 and fp32, one tracer and 25, cold: consecutive calls go to different plans (field sets), as bench.py runs its steps,
so no call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  path       : Plan.column_path, the whole plan, path and mass (two launches)
  path_only  : the same, mass=None (one launch)
  block64    : a block of 64 instances in the middle of the plan, path and mass
  export_f   : Plan.export_device of f alone -- the work a caller does today before a kernel of their own even starts;
               its code is that of the parent commit
and from them GB/s against the nx * nzm * ncrms * elem bytes the reduction has to read, and the ratio path / export_f.
The result of one call is checked against torch on the exported copy (to rounding: torch's sum has another order).
Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/column_path_bench.py [--steps K] [--sets N] [--json PATH] [--no-t25]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--ncrms", type=int, default=65536)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=28)
ap.add_argument("--json", default=None)
ap.add_argument("--no-t25", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
ncrms, nx, nz = a.ncrms, a.nx, a.nz
nzm = nz - 1
out = {"shape": [ncrms, nx, nz], "steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0)}


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps):
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = loop_ms(fn, steps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return min(loop_ms(fn, steps) for _ in range(3))


def measure(tag, tdt, eb, T, sets, steps):
    sh = M.shapes(ncrms, nx, nz, T)
    sh1 = M.shapes(ncrms, nx, nz, 1)
    plans = []
    ftmp = torch.empty(sh1["f"], dtype=tdt, device=dev)
    rho, adz = (torch.empty(sh1[k], dtype=tdt, device=dev) for k in ("rho", "adz"))
    M.fill_synthetic(rho, "rho", 7, 1)
    M.fill_synthetic(adz, "adz", 7, 1)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR
        p.set_stream()
        p.set_timing(False)
        for t in range(T):
            M.fill_synthetic(ftmp, "f", 100 + s * T + t, 1)
            p.import_device(f=ftmp, first_tracer=t)
        p.import_device(rho=rho, adz=adz)
        plans.append(p)
    del ftmp
    lead = T if T > 1 else None
    osh, bsh = M.column_path_shapes(ncrms, nx, lead), M.column_path_shapes(64, nx, lead)
    o = {k: torch.empty(osh[k], dtype=tdt, device=dev) for k in osh}
    ob = {k: torch.empty(bsh[k], dtype=tdt, device=dev) for k in bsh}
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    need = float(nx) * nzm * ncrms * eb * T      # bytes the reduction has to read
    res = {}
    res["path_ms"] = timed(lambda i: plans[i % n].column_path(o["path"], o["mass"]), steps)
    res["path_only_ms"] = timed(lambda i: plans[i % n].column_path(o["path"]), steps)
    res["block64_ms"] = timed(lambda i: plans[i % n].column_path(ob["path"], ob["mass"], ncrms // 2 - 7, 64), steps)
    res["export_f_ms"] = timed(lambda i: plans[i % n].export_device(f=fx), steps)
    res["path_ms_again"] = timed(lambda i: plans[i % n].column_path(o["path"], o["mass"]), steps)
    res["read_bytes"] = need
    res["path_gbs"] = need / res["path_ms"] / 1e6
    res["block64_gbs"] = float(nx) * nzm * 64 * eb * T / res["block64_ms"] / 1e6
    res["ratio_path_over_export"] = res["path_ms"] / res["export_f_ms"]
    # the result against torch on the exported copy, to rounding (another order, and torch may contract)
    plans[0].column_path(o["path"], o["mass"])
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    inner = fx[..., 3:nx + 3, :]                               # ([T,] nzm, nx, ncrms)
    wgt = (rho * adz)[:, None, :]
    ref = (inner * wgt).sum(dim=-3)
    scale = (inner.abs() * wgt).sum(dim=-3).clamp_min(1e-300)
    err = float(((o["path"] - ref).abs() / scale).max())
    assert err < 2 * nzm * (2.3e-16 if eb == 8 else 1.2e-7), (tag, err)
    errm = float(((o["mass"] - o["path"].sum(dim=-2)).abs() / o["path"].abs().sum(dim=-2).clamp_min(1e-300)).max())
    assert errm < nx * (2.3e-16 if eb == 8 else 1.2e-7), (tag, errm)
    plans[0].column_path(ob["path"], ob["mass"], ncrms // 2 - 7, 64)
    torch.cuda.synchronize()
    assert torch.equal(ob["path"], o["path"][..., ncrms // 2 - 7:ncrms // 2 + 57]), tag
    assert torch.equal(ob["mass"], o["mass"][..., ncrms // 2 - 7:ncrms // 2 + 57]), tag
    for p in plans:
        p.close()
    del plans, o, ob, fx
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:10s}: path + mass {res['path_ms']:.4f} ms ({res['path_gbs']:.0f} GB/s of f's interior)  path alone "
          f"{res['path_only_ms']:.4f}  block of 64 {res['block64_ms']:.4f}  export f {res['export_f_ms']:.4f}  "
          f"path / export {res['ratio_path_over_export']:.3f}", flush=True)


M.set_variant(M.VARIANT_FAST)
measure("f64_t1", torch.float64, 8, 1, a.sets, a.steps)
measure("f32_t1", torch.float32, 4, 1, a.sets, a.steps)
if not a.no_t25:
    measure("f64_t25", torch.float64, 8, 25, 2, 6)
    measure("f32_t25", torch.float32, 4, 25, 2, 6)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
