#!/usr/bin/env python3
"""Time of the outflow Courant number of a resident plan's velocities (include/mpdata_hip.h 3h) at ncrms=65536 nx=32
nz=28, one precision per process (--precision f64 | f32), cold: consecutive calls go to different plans (field sets), as
bench.py runs its steps, so no call finds its u, w in the Infinity Cache.  Per call (torch events -- HIP event pairs --
around a loop of K calls on the plans' stream, after a wake-up: batches of calls until two consecutive batch times agree
within 3 %; the minimum of three loops):
  courant      : Plan.courant, the whole plan, clev + cinst
  courant_clev : the same, clev alone;  courant_cinst: cinst alone
  block64      : a block of 64 instances in the middle of the plan, clev + cinst
  array        : courant() on reference-layout device arrays u, w, rho, adz (another set per call), clev + cinst
  level_stats  : Plan.level_stats with all three outputs, one tracer, on the same plans -- the yardstick: unchanged code
                 of the parent commit that streams ONE array of f's size where courant streams two
and from them the ratio courant / level_stats (the bar: <= 3) and GB/s against the bytes of the interior columns of u + w.
The result of plan 0 is also compared bit for bit with the array form on the arrays that were imported.
Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, merges its block into the
file (so that the two precisions, run as two processes each under a time limit of its own and chained with &&, share it):
  timeout -k 10 300 python tools/courant_bench.py --precision f64 --json profiles/courant_bench.json && \\
  timeout -k 10 300 python tools/courant_bench.py --precision f32 --json profiles/courant_bench.json
usage: python tools/courant_bench.py --precision f64|f32 [--steps K] [--sets N] [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=("f64", "f32"), required=True)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--ncrms", type=int, default=65536)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=28)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ncrms, nx, nz = a.ncrms, a.nx, a.nz
nzm = nz - 1
tdt, eb = (torch.float64, 8) if a.precision == "f64" else (torch.float32, 4)


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


M.set_variant(M.VARIANT_FAST)
sh = M.shapes(ncrms, nx, nz, 1)
plans, arrays = [], []
tmp = {k: torch.empty(sh[k], dtype=tdt, device=dev) for k in ("f", "rhow", "flux")}
for s in range(a.sets):
    p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
    assert p.layout == M.LAYOUT_WAVEMAJOR
    p.set_stream()
    p.set_timing(False)
    d = {k: torch.empty(sh[k], dtype=tdt, device=dev) for k in ("u", "w", "rho", "adz")}
    for k in d:
        M.fill_synthetic(d[k], k, 100 + s, 1)
    for k in tmp:
        M.fill_synthetic(tmp[k], k, 100 + s, 1)
    p.import_device(**tmp, **d)
    plans.append(p)
    arrays.append(d)
del tmp
n = len(plans)
lev, ins = torch.empty((nzm, ncrms), dtype=tdt, device=dev), torch.empty((ncrms,), dtype=tdt, device=dev)
levb, insb = torch.empty((nzm, 64), dtype=tdt, device=dev), torch.empty((64,), dtype=tdt, device=dev)
o = [torch.empty((nzm, ncrms), dtype=tdt, device=dev) for _ in range(3)]
torch.cuda.synchronize()

res = {"steps": a.steps, "sets": a.sets}
res["courant_ms"] = timed(lambda i: plans[i % n].courant(clev=lev, cinst=ins), a.steps)
res["courant_clev_ms"] = timed(lambda i: plans[i % n].courant(clev=lev), a.steps)
res["courant_cinst_ms"] = timed(lambda i: plans[i % n].courant(cinst=ins), a.steps)
res["block64_ms"] = timed(lambda i: plans[i % n].courant(ncrms // 2 - 7, 64, clev=levb, cinst=insb), a.steps)
res["level_stats_ms"] = timed(lambda i: plans[i % n].level_stats(sum=o[0], min=o[1], max=o[2]), a.steps)
res["array_ms"] = timed(lambda i: M.courant(clev=lev, cinst=ins, **arrays[i % n]), a.steps)
res["courant_ms_again"] = timed(lambda i: plans[i % n].courant(clev=lev, cinst=ins), a.steps)
res["read_bytes_u_w"] = float(2 * nx + 1) * nzm * ncrms * eb      # columns 1 .. nx+1 of u, 1 .. nx of w
res["courant_gbs"] = res["read_bytes_u_w"] / res["courant_ms"] / 1e6
res["array_gbs"] = res["read_bytes_u_w"] / res["array_ms"] / 1e6
res["ratio_courant_over_level_stats"] = res["courant_ms"] / res["level_stats_ms"]
# plan form against array form, bit for bit
lev2, ins2 = torch.empty_like(lev), torch.empty_like(ins)
plans[0].courant(clev=lev, cinst=ins)
M.courant(clev=lev2, cinst=ins2, **arrays[0])
torch.cuda.synchronize()
assert torch.equal(lev.view(torch.uint8), lev2.view(torch.uint8)) and torch.equal(ins.view(torch.uint8), ins2.view(torch.uint8))
assert torch.equal(ins, lev.amax(dim=0)) and float(ins.max()) > 0
res["max_cinst"] = float(ins.max())
for p in plans:
    p.close()
print(f"{a.precision}: courant {res['courant_ms']:.4f} ms ({res['courant_gbs']:.0f} GB/s of u + w)  clev alone "
      f"{res['courant_clev_ms']:.4f}  cinst alone {res['courant_cinst_ms']:.4f}  block of 64 {res['block64_ms']:.4f}  "
      f"level stats {res['level_stats_ms']:.4f}  courant / level stats {res['ratio_courant_over_level_stats']:.3f}  "
      f"array form {res['array_ms']:.4f} ({res['array_gbs']:.0f} GB/s)", flush=True)
out = {}
if a.json and os.path.exists(a.json):
    with open(a.json) as fh:
        out = json.load(fh)
out.update({"shape": [ncrms, nx, nz], "device": torch.cuda.get_device_name(0), a.precision: res})
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
