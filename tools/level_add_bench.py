#!/usr/bin/env python3
"""Time of the per-level increments of a resident plan (include/mpdata_hip.h 3i) at ncrms=65536 nx=32 nz=28, fp64 and
fp32, one tracer and 25, cold: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no
call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  add        : Plan.level_add, the whole plan, MPDATA_LEVEL_ADD
  add_clip   : the same, MPDATA_LEVEL_ADD_CLIP
  block64    : a block of 64 instances in the middle of the plan
  export_import_f : Plan.export_device of f alone followed by Plan.import_device of the copy -- the cheapest way a caller
               had before, even without the kernel of their own in between; this code is that of the parent commit
and from them GB/s against the 2 * (nx + 6) * nzm * ncrms * elem bytes the call has to read and write, and the ratio
add / export_import_f.  The result is compared bit for bit with torch on the exported copies.
Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/level_add_bench.py [--steps K] [--sets N] [--json PATH] [--no-t25]"""
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
    dshape = ((T,) if T > 1 else ()) + (nzm, ncrms)
    # increments of 1e-3 of f's size, both signs: thousands of calls leave f where it was
    d = ((torch.rand(dshape, dtype=torch.float64, device=dev) - 0.5) * 2e-3).to(tdt)
    db = d[..., ncrms // 2 - 7:ncrms // 2 + 57].contiguous()
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    need = 2.0 * (nx + 6) * nzm * ncrms * eb * T      # bytes the call has to read and write

    def export_import(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    res = {}
    res["add_ms"] = timed(lambda i: plans[i % n].level_add(d), steps)
    res["add_clip_ms"] = timed(lambda i: plans[i % n].level_add(d, mode=M.LEVEL_ADD_CLIP), steps)
    res["block64_ms"] = timed(lambda i: plans[i % n].level_add(db, ncrms // 2 - 7, 64), steps)
    res["export_import_f_ms"] = timed(export_import, steps)
    res["add_ms_again"] = timed(lambda i: plans[i % n].level_add(d), steps)
    res["rw_bytes"] = need
    res["add_gbs"] = need / res["add_ms"] / 1e6
    res["ratio_add_over_export_import"] = res["add_ms"] / res["export_import_f_ms"]
    # the result against torch on the exported copies, bit for bit (one rounded add; the max of a non-zero sum)
    for mode in (M.LEVEL_ADD, M.LEVEL_ADD_CLIP):
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        want = fx + d.unsqueeze(-2)
        if mode == M.LEVEL_ADD_CLIP:
            want = want.clamp_min(0)
        plans[0].level_add(d, mode=mode)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        assert torch.equal(fx, want), (tag, mode)
        del want
    for p in plans:
        p.close()
    del plans, d, db, fx
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:10s}: add {res['add_ms']:.4f} ms ({res['add_gbs']:.0f} GB/s read + written)  clip {res['add_clip_ms']:.4f}  "
          f"block of 64 {res['block64_ms']:.4f}  export + import f {res['export_import_f_ms']:.4f}  "
          f"add / (export + import) {res['ratio_add_over_export_import']:.3f}", flush=True)


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
