#!/usr/bin/env python3
"""Time of the eddy diffusion of a resident plan (include/mpdata_hip.h 3l) at ncrms=65536 nx=32 nz=28, fp64, one tracer,
cold: consecutive calls go to different plans (field sets) with their own tkh, as bench.py runs its steps, so no call finds
its f or its tkh in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  diffuse       : Plan.diffuse, the whole plan, sb = st = zflux = None (the conversion pass of tkh and the kernel)
  diffuse_full  : the same with sb, st and zflux
  block64       : a block of 64 instances in the middle of the plan
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel; its code is that of the parent commit
and from them the ratio diffuse / round_trip and GB/s against two byte counts: the algorithmic traffic (f's nx + 2 columns
read and nx written, tkh's nx + 2 columns read) and the traffic with the conversion pass of tkh (its nx + 2 columns read
and written once more).  The result of one call is checked against torch on the exported copies (to rounding: torch may
contract and associates differently).  Needs no oracle and no reference tree.  Prints one line per measurement and, with
--json PATH, writes them all there.
usage: python tools/diffuse_bench.py [--steps K] [--sets N] [--json PATH] [--f32]"""
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
    dsh, bsh = M.diffuse_shapes(ncrms, nx, nz), M.diffuse_shapes(64, nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    rho, adz = rnd(sh["rho"], 0.5, 1.0), rnd(sh["adz"], 0.5, 1.0)
    cx, cz = rnd(dsh["cx"], 1 / 32, 1 / 16), rnd(dsh["cz"], 1 / 128, 1 / 64)
    sb, st = rnd(dsh["sb"], -1 / 64, 1 / 64), rnd(dsh["st"], -1 / 64, 1 / 64)
    zflux = torch.empty(dsh["zflux"], dtype=tdt, device=dev)
    plans, tkhs = [], []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp, rho=rho, adz=adz)
        plans.append(p)
        tkhs.append(rnd(dsh["tkh"], 0.5, 1.0))
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    blk = {k: (v[..., ncrms // 2 - 7:ncrms // 2 + 57].contiguous() if v is not None else None)
           for k, v in (("tkh", tkhs[0]), ("cx", cx), ("cz", cz))}
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                       # bytes of one column of all instances
    alg = col * ((nx + 2) + nx + (nx + 2))              # f read, f written, tkh read
    conv = col * 2 * (nx + 2)                           # tkh read and written once more by the conversion pass
    res = {"algorithmic_bytes": alg, "conversion_bytes": conv, "round_trip_bytes": col * 4 * (nx + 6)}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on diffusing the same fields): one call against torch on the exported copies
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    f0 = fx.clone()
    plans[0].diffuse(tkhs[0], cx, cz, sb, st, zflux)
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    c = f0[:, 2:nx + 4].double()                        # (nzm, nx+2, ncrms): columns 0 .. nx+1
    tk = tkhs[0].double()
    fxx = -(cx.double()[:, None] * (tk[:, :-1] + tk[:, 1:])) * (c[:, 1:] - c[:, :-1])
    fz = torch.zeros((nzm + 1, nx, ncrms), dtype=torch.float64, device=dev)
    fz[1:nzm] = -(cz.double()[:-1, None] * (tk[:-1, 1:-1] + tk[1:, 1:-1])) * (c[1:, 1:-1] - c[:-1, 1:-1])
    fz[0], fz[nzm] = sb.double(), st.double()
    ir = 1.0 / (rho.double() * adz.double())
    ref = c[:, 1:-1] - ((fxx[:, 1:] - fxx[:, :-1]) + (fz[1:] - fz[:-1]) * ir[:, None])
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    err = float((fx[:, 3:nx + 3].double() - ref).abs().max() / c.abs().max())
    assert err < 64 * eps, (tag, err)
    errz = float((zflux.double() - fz.sum(dim=1)).abs().max() / fz.abs().sum(dim=1).max())
    assert errz < 2 * nx * eps, (tag, errz)
    assert torch.equal(fx[:, :3], f0[:, :3]) and torch.equal(fx[:, nx + 3:], f0[:, nx + 3:]), tag
    del f0, c, tk, fxx, fz, ref
    torch.cuda.empty_cache()

    res["diffuse_ms"] = timed(lambda i: plans[i % n].diffuse(tkhs[i % n], cx, cz), steps)
    res["diffuse_full_ms"] = timed(lambda i: plans[i % n].diffuse(tkhs[i % n], cx, cz, sb, st, zflux), steps)
    res["block64_ms"] = timed(lambda i: plans[i % n].diffuse(blk["tkh"], blk["cx"], blk["cz"], sl0=ncrms // 2 - 7, n=64), steps)
    res["round_trip_ms"] = timed(round_trip, steps)
    res["diffuse_ms_again"] = timed(lambda i: plans[i % n].diffuse(tkhs[i % n], cx, cz), steps)
    res["ratio_diffuse_over_round_trip"] = res["diffuse_ms"] / res["round_trip_ms"]
    res["algorithmic_gbs"] = alg / res["diffuse_ms"] / 1e6
    res["moved_gbs"] = (alg + conv) / res["diffuse_ms"] / 1e6
    res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
    for p in plans:
        p.close()
    del plans, tkhs, fx
    torch.cuda.empty_cache()
    out[tag] = res
    print(f"{tag:7s}: diffuse {res['diffuse_ms']:.4f} ms ({res['algorithmic_gbs']:.0f} GB/s algorithmic, {res['moved_gbs']:.0f} GB/s "
          f"with the tkh conversion)  with sb, st, zflux {res['diffuse_full_ms']:.4f}  block of 64 {res['block64_ms']:.4f}  "
          f"export + import of f {res['round_trip_ms']:.4f}  diffuse / round trip {res['ratio_diffuse_over_round_trip']:.3f}", flush=True)


M.set_variant(M.VARIANT_FAST)
measure("f64_t1", torch.float64, 8, a.sets, a.steps)
if a.f32:
    measure("f32_t1", torch.float32, 4, a.sets, a.steps)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
