#!/usr/bin/env python3
"""Time of the level statistics of a resident plan (include/mpdata_hip.h 3g) at ncrms=65536 nx=32 nz=28, fp64 and
fp32, one tracer and 25, cold: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no
call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  stats      : Plan.level_stats, the whole plan, sum + min + max
  stats_sum  : the same, sum alone
  block64    : a block of 64 instances in the middle of the plan
  export_f   : Plan.export_device of f alone -- the first half of what a caller had to do before (export, then reduce
               the reference-layout copy); its code is that of the parent commit
and from them GB/s against the nx * nzm * ncrms * elem bytes the reduction has to read, and the ratio stats / export_f.
Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/level_stats_bench.py [--steps K] [--sets N] [--json PATH] [--no-t25]"""
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
    plans = []
    ftmp = torch.empty(M.shapes(ncrms, nx, nz, 1)["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR
        p.set_stream()
        p.set_timing(False)
        for t in range(T):
            M.fill_synthetic(ftmp, "f", 100 + s * T + t, 1)
            p.import_device(f=ftmp, first_tracer=t)
        plans.append(p)
    del ftmp
    oshape = ((T,) if T > 1 else ()) + (nzm, ncrms)
    o = [torch.empty(oshape, dtype=tdt, device=dev) for _ in range(3)]
    ob = [torch.empty(((T,) if T > 1 else ()) + (nzm, 64), dtype=tdt, device=dev) for _ in range(3)]
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    need = float(nx) * nzm * ncrms * eb * T      # bytes the reduction has to read
    res = {}
    res["stats_ms"] = timed(lambda i: plans[i % n].level_stats(sum=o[0], min=o[1], max=o[2]), steps)
    res["stats_sum_ms"] = timed(lambda i: plans[i % n].level_stats(sum=o[0]), steps)
    res["block64_ms"] = timed(lambda i: plans[i % n].level_stats(ncrms // 2 - 7, 64, sum=ob[0], min=ob[1], max=ob[2]), steps)
    res["export_f_ms"] = timed(lambda i: plans[i % n].export_device(f=fx), steps)
    res["stats_ms_again"] = timed(lambda i: plans[i % n].level_stats(sum=o[0], min=o[1], max=o[2]), steps)
    res["read_bytes"] = need
    res["stats_gbs"] = need / res["stats_ms"] / 1e6
    res["ratio_stats_over_export"] = res["stats_ms"] / res["export_f_ms"]
    # the result against torch on the exported copy (order-free quantities bitwise, the sum to rounding)
    plans[0].level_stats(sum=o[0], min=o[1], max=o[2])
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    inner = fx[..., 3:nx + 3, :]
    assert torch.equal(o[1], inner.amin(dim=-2)) and torch.equal(o[2], inner.amax(dim=-2)), tag
    err = float(((o[0] - inner.sum(dim=-2)).abs() / inner.abs().sum(dim=-2).clamp_min(1e-300)).max())
    assert err < nx * (2.3e-16 if eb == 8 else 1.2e-7), (tag, err)
    for p in plans:
        p.close()
    del plans, o, ob, fx
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:10s}: stats {res['stats_ms']:.4f} ms ({res['stats_gbs']:.0f} GB/s of f's interior)  sum alone "
          f"{res['stats_sum_ms']:.4f}  block of 64 {res['block64_ms']:.4f}  export f {res['export_f_ms']:.4f}  "
          f"stats / export {res['ratio_stats_over_export']:.3f}", flush=True)


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
