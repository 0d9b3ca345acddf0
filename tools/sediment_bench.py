#!/usr/bin/env python3
"""Time of the sedimentation of a resident plan (include/mpdata_hip.h 3n) at ncrms=65536 nx=32 nz=28, one tracer, cold:
consecutive calls go to different plans (field sets) with their own wp, as bench.py runs its steps, so no call finds its f
or its wp in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a wake-up:
batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  sediment      : Plan.sediment, the whole plan, psfc = pflux = None
  sediment_out  : the same with psfc and pflux
  block64       : a block of 64 instances in the middle of the plan (odd sl0: partial rows of wp)
and three yardsticks in the same process, all of them code of the parent commit:
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel
  level_add     : Plan.level_add -- reads and writes every column slot of f, no per-cell field
  diffuse       : Plan.diffuse, sb = st = zflux = None -- carries a conversion pass for a per-cell field of wp's size
and from them the three ratios and GB/s against the bytes each call moves: sediment its algorithmic traffic (the interior
of f read once and written once, wp read once: 3 nx nzm ncrms reals), level_add 2 (nx + 6) columns, the round trip twice
that, diffuse its algorithmic traffic plus the conversion pass of tkh.  The result of one call is checked against torch on
the exported copies (to rounding: torch may contract).  Needs no oracle and no reference tree.  Prints one line per
measurement and, with --json PATH, writes them all there.
usage: python tools/sediment_bench.py [--steps K] [--sets N] [--json PATH] [--f32]"""
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
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler): sediment, sediment_out, diffuse")
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
    ssh = M.sediment_shapes(ncrms, nx, nz)
    dsh = M.diffuse_shapes(ncrms, nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    # (small coefficients of both signs: hundreds of timed calls on one field stay finite)
    psfc = torch.empty(ssh["psfc"], dtype=tdt, device=dev)
    pflux = torch.empty(ssh["pflux"], dtype=tdt, device=dev)
    d = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
    cx, cz = rnd(dsh["cx"], 1e-4, 2e-4), rnd(dsh["cz"], 1e-4, 2e-4)
    plans, wps, tkhs, first = [], [], [], {}
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp)
        for k in ("rho", "adz"):
            t = rnd(sh[k], 0.5, 1.0)
            p.import_device(**{k: t})
            if s == 0:
                first[k] = t
        plans.append(p)
        wps.append(rnd(ssh["wp"], -0.002, 0.008))
        tkhs.append(rnd(dsh["tkh"], 0.5, 1.0))
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    lo = ncrms // 2 - 7
    bwp = wps[0][:, :, lo:lo + 64].contiguous()
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances
    alg = col * 3 * nx                                   # the interior of f read and written, wp read
    res = {"algorithmic_bytes": alg, "level_add_bytes": col * 2 * (nx + 6), "round_trip_bytes": col * 4 * (nx + 6),
           "diffuse_moved_bytes": col * ((nx + 2) + nx + (nx + 2) + 2 * (nx + 2))}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on changing the same fields): one call against torch on the exported copies
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    f0 = fx.clone().double()                              # (nzm, nx+6, ncrms); a copy also where fx is float64
    plans[0].sediment(wps[0], psfc, pflux)
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    ir = 1.0 / (first["rho"].double() * first["adz"].double())
    fz = wps[0].double() * f0[:, 3:nx + 3]
    fzu = torch.cat([fz[1:], torch.zeros_like(fz[:1])])
    want = f0.clone()
    want[:, 3:nx + 3] -= (fz - fzu) * ir[:, None]
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    err = float((fx.double() - want).abs().max() / f0.abs().max())
    assert err < 8 * eps, (tag, err)
    errs = float((psfc.double() - fz[0]).abs().max() / fz[0].abs().max())
    errp = float((pflux.double() - fz.sum(dim=1)).abs().max() / fz.abs().sum(dim=1).max())
    assert errs < 2 * eps and errp < 2 * nx * eps, (tag, errs, errp)
    del f0, fz, fzu, want, ir, first
    torch.cuda.empty_cache()

    runs = {
        "sediment": lambda i: plans[i % n].sediment(wps[i % n]),
        "sediment_out": lambda i: plans[i % n].sediment(wps[i % n], psfc, pflux),
        "block64": lambda i: plans[i % n].sediment(bwp, sl0=lo, n=64),
        "round_trip": round_trip,
        "level_add": lambda i: plans[i % n].level_add(d),
        "diffuse": lambda i: plans[i % n].diffuse(tkhs[i % n], cx, cz),
    }
    if a.only:
        res[a.only + "_ms"] = timed(runs[a.only], steps)
        print(f"{tag:7s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"] = timed(fn, steps)
        res["sediment_ms_again"] = timed(runs["sediment"], steps)
        for k in ("round_trip", "level_add", "diffuse"):
            res["ratio_sediment_over_" + k] = res["sediment_ms"] / res[k + "_ms"]
        res["sediment_gbs"] = alg / res["sediment_ms"] / 1e6
        res["level_add_gbs"] = res["level_add_bytes"] / res["level_add_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        res["diffuse_moved_gbs"] = res["diffuse_moved_bytes"] / res["diffuse_ms"] / 1e6
        print(f"{tag:7s}: sediment {res['sediment_ms']:.4f} ms ({res['sediment_gbs']:.0f} GB/s)  with psfc, pflux "
              f"{res['sediment_out_ms']:.4f}  block of 64 {res['block64_ms']:.4f}  export + import of f {res['round_trip_ms']:.4f} "
              f"({res['round_trip_gbs']:.0f} GB/s)  level_add {res['level_add_ms']:.4f} ({res['level_add_gbs']:.0f} GB/s)  diffuse "
              f"{res['diffuse_ms']:.4f} ({res['diffuse_moved_gbs']:.0f} GB/s moved)  sediment / round trip "
              f"{res['ratio_sediment_over_round_trip']:.3f}  / level_add {res['ratio_sediment_over_level_add']:.3f}  / diffuse "
              f"{res['ratio_sediment_over_diffuse']:.3f}", flush=True)
    for p in plans:
        p.close()
    del plans, wps, tkhs, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
measure("f64_t1", torch.float64, 8, a.sets, a.steps)
if a.f32:
    measure("f32_t1", torch.float32, 4, a.sets, a.steps)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
