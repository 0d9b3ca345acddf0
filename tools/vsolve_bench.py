#!/usr/bin/env python3
"""Time of the implicit vertical solve of a resident plan (include/mpdata_hip.h 3o) at ncrms=65536 nx=32 nz=28, one
tracer, cold: consecutive calls go to different plans (field sets) with their own coefficients, as bench.py runs its
steps, so no call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream,
after a wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %):
  vsolve        : Plan.vsolve, the whole plan (the factor kernel included)
  block64       : a block of 64 instances in the middle of the plan (odd sl0)
and three yardsticks in the same process, all of them code of the parent commit:
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel
  column_path   : Plan.column_path, mass = None -- the same staging through LDS, read only
  level_add     : Plan.level_add -- reads and writes every column slot of f, no staging
and from them the three ratios and GB/s against the bytes each call moves: vsolve its algorithmic traffic (the interior of
f read once and written once: 2 nx nzm ncrms reals), column_path half of that, level_add 2 (nx + 6) columns, the round
trip twice that.  With --tall NZ the same four on a windowed plan of NZ levels and --tall-ncrms instances (two passes over
f are expected to cost about twice the plain time per byte).  The result of one call is checked against a Thomas solve in
torch float64 on the exported copies (to rounding).  Needs no oracle and no reference tree.  Prints one line per measurement
and, with --json PATH, writes them all there.
usage: python tools/vsolve_bench.py [--steps K] [--sets N] [--json PATH] [--f32] [--tall 300]"""
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
ap.add_argument("--tall", type=int, default=0, help="a windowed plan of this many levels as well (0: none)")
ap.add_argument("--tall-ncrms", type=int, default=4096)
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler): vsolve, column_path, ...")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"shape": [a.ncrms, a.nx, a.nz], "steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0)}


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


def measure(tag, tdt, eb, ncrms, nx, nz, sets, steps, tall=False):
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, 1)
    vsh = M.vsolve_shapes(ncrms, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    d = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
    path = torch.empty(M.column_path_shapes(ncrms, nx)["path"], dtype=tdt, device=dev)
    plans, cs = [], []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp)
        for k in ("rho", "adz"):
            p.import_device(**{k: rnd(sh[k], 0.5, 1.0)})
        plans.append(p)
        # (diagonally dominant, |inverse| <= 1: hundreds of timed calls on one field stay finite)
        lo, up = rnd(vsh["lo"], -0.4, 0.0), rnd(vsh["up"], -0.4, 0.0)
        cs.append((lo, (1.0 - lo.double() - up.double()).to(tdt), up))
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    b0 = ncrms // 2 - 7
    bc = tuple(t[:, b0:b0 + 64].contiguous() for t in cs[0])
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances
    alg = col * 2 * nx                                   # the interior of f read and written
    res = {"shape": [ncrms, nx, nz], "algorithmic_bytes": alg, "column_path_bytes": col * nx, "level_add_bytes": col * 2 * (nx + 6),
           "round_trip_bytes": col * 4 * (nx + 6), "level_windows": plans[0].level_windows}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on changing the same fields): one call against a Thomas solve in float64
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    f0 = fx.clone().double()                              # (nzm, nx+6, ncrms)
    plans[0].vsolve(*cs[0])
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    lo, di, up = (t.double() for t in cs[0])
    y = f0[:, 3:nx + 3].clone()
    gk = torch.zeros_like(di)
    pk = 1.0 / di[0]
    y[0] *= pk
    gk[0] = up[0] * pk
    for k in range(1, nzm):
        pk = 1.0 / (di[k] - lo[k] * gk[k - 1])
        gk[k] = up[k] * pk
        y[k] = (y[k] - lo[k] * y[k - 1]) * pk
    for k in range(nzm - 2, -1, -1):
        y[k] -= gk[k] * y[k + 1]
    want = f0.clone()
    want[:, 3:nx + 3] = y
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    err = float((fx.double() - want).abs().max() / f0.abs().max())
    assert err < 16 * eps, (tag, err)
    del f0, y, gk, want, lo, di, up
    torch.cuda.empty_cache()

    runs = {
        "vsolve": lambda i: plans[i % n].vsolve(*cs[i % n]),
        "block64": lambda i: plans[i % n].vsolve(*bc, sl0=b0, n=64),
        "round_trip": round_trip,
        "column_path": lambda i: plans[i % n].column_path(path),
        "level_add": lambda i: plans[i % n].level_add(d),
    }
    if a.only:
        res[a.only + "_ms"] = timed(runs[a.only], steps)
        print(f"{tag:7s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"] = timed(fn, steps)
        res["vsolve_ms_again"] = timed(runs["vsolve"], steps)
        for k in ("round_trip", "column_path", "level_add"):
            res["ratio_vsolve_over_" + k] = res["vsolve_ms"] / res[k + "_ms"]
        res["vsolve_gbs"] = alg / res["vsolve_ms"] / 1e6
        res["column_path_gbs"] = res["column_path_bytes"] / res["column_path_ms"] / 1e6
        res["level_add_gbs"] = res["level_add_bytes"] / res["level_add_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        print(f"{tag:9s}: vsolve {res['vsolve_ms']:.4f} ms ({res['vsolve_gbs']:.0f} GB/s)  block of 64 {res['block64_ms']:.4f}  "
              f"export + import of f {res['round_trip_ms']:.4f} ({res['round_trip_gbs']:.0f} GB/s)  column_path "
              f"{res['column_path_ms']:.4f} ({res['column_path_gbs']:.0f} GB/s)  level_add {res['level_add_ms']:.4f} "
              f"({res['level_add_gbs']:.0f} GB/s)  vsolve / round trip {res['ratio_vsolve_over_round_trip']:.3f}  / column_path "
              f"{res['ratio_vsolve_over_column_path']:.3f}  / level_add {res['ratio_vsolve_over_level_add']:.3f}", flush=True)
    for p in plans:
        p.close()
    del plans, cs, fx
    torch.cuda.empty_cache()
    M.set_tall_columns(0)
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
measure("f64_t1", torch.float64, 8, a.ncrms, a.nx, a.nz, a.sets, a.steps)
if a.f32:
    measure("f32_t1", torch.float32, 4, a.ncrms, a.nx, a.nz, a.sets, a.steps)
if a.tall:
    measure("f64_tall", torch.float64, 8, a.tall_ncrms, a.nx, a.tall, min(a.sets, 3), a.steps, tall=True)
    if a.f32:
        measure("f32_tall", torch.float32, 4, a.tall_ncrms, a.nx, a.tall, min(a.sets, 3), a.steps, tall=True)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
