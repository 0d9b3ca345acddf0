#!/usr/bin/env python3
"""Time of the per-instance scaling of a resident plan's velocities (include/mpdata_hip.h 3j) at ncrms=65536 nx=32
nz=28, fp64 and fp32, cold: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no call
finds its u, w in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  scale      : Plan.scale_uw, the whole plan, su and sw (two launches)
  scale_u    : the same, su alone
  block64    : a block of 64 instances in the middle of the plan, su and sw
  import_uw  : Plan.import_device of u and w alone from reference-layout device arrays -- what a caller had before (with
               a second copy of u, w and a scaling kernel of their own in front of it, not timed here); this code is
               that of the parent commit
and from them GB/s against the 2 * ((nx + 5) + (nx + 4)) * nzm * ncrms * elem bytes the call has to read and write, and
the ratio scale / import_uw.  The factors are powers of two, a set and its reciprocals in turn on every plan, so
thousands of calls leave u, w where they were.  The result is compared bit for bit through the Courant number:
Plan.courant after a scaling by factors of 1/3 and 3/7 against courant() on the torch-scaled reference-layout arrays.
Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/scale_uw_bench.py [--steps K] [--sets N] [--json PATH]"""
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
    plans, arrays = [], []
    tmp = {k: torch.empty(sh[k], dtype=tdt, device=dev) for k in ("f", "rhow", "flux")}
    for s in range(sets):
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
    # powers of two and their reciprocals: exact, and applied in turn they restore every bit
    e = torch.randint(0, 4, (ncrms,), device=dev)
    s_a = torch.pow(torch.tensor(2.0, dtype=tdt, device=dev), -e.to(tdt))
    s_b = torch.pow(torch.tensor(2.0, dtype=tdt, device=dev), e.to(tdt))
    b0 = ncrms // 2 - 7
    sb_a, sb_b = s_a[b0:b0 + 64].contiguous(), s_b[b0:b0 + 64].contiguous()
    torch.cuda.synchronize()
    n = len(plans)
    calls = [0] * n

    def turn(i, x, y):            # every plan takes the set and its reciprocals in turn
        calls[i % n] += 1
        return x if calls[i % n] % 2 else y

    def scale(i, x, y, u_only=False, block=()):
        s = turn(i, x, y)
        plans[i % n].scale_uw(s, None if u_only else s, *block)

    need = 2.0 * ((nx + 5) + (nx + 4)) * nzm * ncrms * eb      # bytes the call has to read and write

    res = {}
    res["scale_ms"] = timed(lambda i: scale(i, s_a, s_b), steps)
    res["scale_u_ms"] = timed(lambda i: scale(i, s_a, s_b, u_only=True), steps)
    res["block64_ms"] = timed(lambda i: scale(i, sb_a, sb_b, block=(b0, 64)), steps)
    res["import_uw_ms"] = timed(lambda i: plans[i % n].import_device(u=arrays[i % n]["u"], w=arrays[i % n]["w"]), steps)
    res["scale_ms_again"] = timed(lambda i: scale(i, s_a, s_b), steps)
    res["rw_bytes"] = need
    res["scale_gbs"] = need / res["scale_ms"] / 1e6
    res["ratio_scale_over_import_uw"] = res["scale_ms"] / res["import_uw_ms"]
    # the result through the Courant number, bit for bit (one rounded multiply; 1/3 and 3/7 make the product round)
    p, d = plans[0], arrays[0]
    p.import_device(u=d["u"], w=d["w"])
    su = torch.where(e % 2 == 0, torch.tensor(1.0 / 3.0, dtype=tdt, device=dev), torch.tensor(3.0 / 7.0, dtype=tdt, device=dev))
    sw = torch.where(e < 2, torch.tensor(1.0 / 5.0, dtype=tdt, device=dev), torch.tensor(0.5, dtype=tdt, device=dev))
    p.scale_uw(su, sw)
    lev, ins = torch.empty((nzm, ncrms), dtype=tdt, device=dev), torch.empty((ncrms,), dtype=tdt, device=dev)
    lev2, ins2 = torch.empty_like(lev), torch.empty_like(ins)
    p.courant(clev=lev, cinst=ins)
    M.courant(d["u"] * su, d["w"] * sw, d["rho"], d["adz"], clev=lev2, cinst=ins2)
    torch.cuda.synchronize()
    assert torch.equal(lev.view(torch.uint8), lev2.view(torch.uint8)) and torch.equal(ins.view(torch.uint8), ins2.view(torch.uint8)), tag
    for p in plans:
        p.close()
    del plans, arrays
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:6s}: scale {res['scale_ms']:.4f} ms ({res['scale_gbs']:.0f} GB/s read + written)  su alone {res['scale_u_ms']:.4f}  "
          f"block of 64 {res['block64_ms']:.4f}  import u, w {res['import_uw_ms']:.4f}  "
          f"scale / import {res['ratio_scale_over_import_uw']:.3f}  (again {res['scale_ms_again']:.4f})", flush=True)


M.set_variant(M.VARIANT_FAST)
measure("f64", torch.float64, 8, a.sets, a.steps)
measure("f32", torch.float32, 4, a.sets, a.steps)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
