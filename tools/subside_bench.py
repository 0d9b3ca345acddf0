#!/usr/bin/env python3
"""Time of the large-scale vertical advection of a resident plan (include/mpdata_hip.h 3m) at ncrms=65536 nx=32 nz=28, one
tracer, cold: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no call finds its f in
the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a wake-up: batches of
calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  subside       : Plan.subside, the whole plan, dsum = None
  subside_dsum  : the same with dsum
  block64       : a block of 64 instances in the middle of the plan
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel; its code is that of the parent commit
  level_add     : Plan.level_add -- the same bytes, 2 (nx + 6) nzm ncrms elements, without the stencil; parent code too
and from them the ratios subside / round_trip and subside / level_add, and GB/s against the algorithmic traffic (every
column slot of f read once and written once).  The result of one call is checked against torch on the exported copies (to
rounding: torch may contract).  Needs no oracle and no reference tree.  Prints one line per measurement and, with
--json PATH, writes them all there.
usage: python tools/subside_bench.py [--steps K] [--sets N] [--json PATH] [--f32]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--ncrms", type=int, default=65536)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=28)
ap.add_argument("--json", default=None)
ap.add_argument("--f32", action="store_true", help="fp32 as well")
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


def measure(tag, tdt, eb, sets, steps):
    sh = M.shapes(ncrms, nx, nz, 1)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    # (small coefficients of both signs: hundreds of timed calls on one field stay finite)
    cb, cc = rnd((nzm, ncrms), -0.01, 0.01), rnd((nzm, ncrms), -0.01, 0.01)
    dsum = torch.empty((nzm, ncrms), dtype=tdt, device=dev)
    d = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
    plans = []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp)
        plans.append(p)
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    lo = ncrms // 2 - 7
    bcb, bcc = cb[:, lo:lo + 64].contiguous(), cc[:, lo:lo + 64].contiguous()
    torch.cuda.synchronize()
    n = len(plans)
    alg = 2.0 * (nx + 6) * nzm * ncrms * eb               # every column slot of f read and written
    res = {"algorithmic_bytes": alg, "round_trip_bytes": 2 * alg}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on advecting the same fields): one call against torch on the exported copies
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    f0 = fx.clone().double()                              # (nzm, nx+6, ncrms); a copy also where fx is float64
    plans[0].subside(cb, cc, dsum)
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    fd = torch.cat([f0[:1], f0[:-1]])
    fu = torch.cat([f0[1:], f0[-1:]])
    dec = cb.double()[:, None] * (f0 - fd) + cc.double()[:, None] * (fu - f0)
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    err = float((fx.double() - (f0 - dec)).abs().max() / f0.abs().max())
    assert err < 8 * eps, (tag, err)
    errd = float((dsum.double() - dec[:, 3:nx + 3].sum(dim=1)).abs().max() / dec[:, 3:nx + 3].abs().sum(dim=1).max())
    assert errd < 2 * nx * eps, (tag, errd)
    del f0, fd, fu, dec
    torch.cuda.empty_cache()

    res["subside_ms"] = timed(lambda i: plans[i % n].subside(cb, cc), steps)
    res["subside_dsum_ms"] = timed(lambda i: plans[i % n].subside(cb, cc, dsum), steps)
    res["block64_ms"] = timed(lambda i: plans[i % n].subside(bcb, bcc, sl0=lo, n=64), steps)
    res["round_trip_ms"] = timed(round_trip, steps)
    res["level_add_ms"] = timed(lambda i: plans[i % n].level_add(d), steps)
    res["subside_ms_again"] = timed(lambda i: plans[i % n].subside(cb, cc), steps)
    res["ratio_subside_over_round_trip"] = res["subside_ms"] / res["round_trip_ms"]
    res["ratio_subside_over_level_add"] = res["subside_ms"] / res["level_add_ms"]
    res["subside_gbs"] = alg / res["subside_ms"] / 1e6
    res["level_add_gbs"] = alg / res["level_add_ms"] / 1e6
    res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
    for p in plans:
        p.close()
    del plans, fx
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:7s}: subside {res['subside_ms']:.4f} ms ({res['subside_gbs']:.0f} GB/s)  with dsum {res['subside_dsum_ms']:.4f}  "
          f"block of 64 {res['block64_ms']:.4f}  export + import of f {res['round_trip_ms']:.4f}  level_add {res['level_add_ms']:.4f}  "
          f"subside / round trip {res['ratio_subside_over_round_trip']:.3f}  subside / level_add "
          f"{res['ratio_subside_over_level_add']:.3f}", flush=True)


M.set_variant(M.VARIANT_FAST)
measure("f64_t1", torch.float64, 8, a.sets, a.steps)
if a.f32:
    measure("f32_t1", torch.float32, 4, a.sets, a.steps)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
