#!/usr/bin/env python3
"""Time of the running column integrals of the tracers of a resident plan (include/mpdata_hip.h 3aa), cold, at ncrms=65536
nx=32 nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), three tracers, fp64 and fp32: consecutive calls go to
different plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch
events around a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped
falling, i.e. two consecutive batches agree within 3 %; then the median, the minimum and the maximum of five rounds, and
their spread (max - min) / median):
  scan_<mode>          : Plan.column_scan of tracer 0 into tracer 1 (dst != src), the whole plan, with wgt and total, in the
                         four modes up, down, up_excl, down_excl
  scan_<mode>_inplace  : the same with dst == src (tracer 2; the field is rescaled by an untimed level_add-free import
                         between rounds, so it stays finite)
  scan_up_nowgt        : without wgt (rho * adz of the plan) and without total
and the yardsticks in the same process on the same plans, all of them calls that exist without 3aa:
  vsolve      : Plan.vsolve of one tracer -- the same staging, two sweeps, a factor kernel in front
  column_path : Plan.column_path of one tracer -- the same staging, read only
  level_add   : Plan.level_add of one tracer -- the same bytes, no staging
  round_trip  : Plan.export_device + Plan.import_device of the tracer -- the route a caller had before the call existed,
                without the caller's own kernel
and from them the ratios and TB/s against the algorithmic bytes: the interior of one tracer read and one written, 2 nx nzm
ncrms reals.  A difference between two measurements below the larger of their spreads is reported as unresolved.  One call
per mode is checked against torch.cumsum on the exported copies first (to rounding: torch sums in another association).
Needs no oracle and no reference tree.
usage: python tools/column_scan_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--only NAME]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--only", default=None, help="time one measurement alone (a profiler)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0), "library": os.path.basename(M.lib_path())}
T = 3
MODES = {"up": 0, "down": M.COLUMN_SCAN_DOWN, "up_excl": M.COLUMN_SCAN_EXCLUSIVE, "down_excl": M.COLUMN_SCAN_DOWN | M.COLUMN_SCAN_EXCLUSIVE}


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps, between=None):
    """-> (median, min, max) of five rounds behind the wake-up; between(): untimed, in front of every round"""
    def one():
        if between:
            between()
            torch.cuda.synchronize()
        return loop_ms(fn, steps)
    prev = one()
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = one()
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    t = [one() for _ in range(5)]
    return statistics.median(t), min(t), max(t)


def measure(tag, shape, tdt, eb, sets, steps, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    sh = M.column_scan_shapes(ncrms, nx, nz)
    wgt = rnd(sh["wgt"], 0.25, 1.0)
    total = torch.empty(sh["total"], dtype=tdt, device=dev)
    plans = []
    one = torch.empty(M.shapes(ncrms, nx, nz, 1)["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        for t in range(T):
            M.fill_synthetic(one, "f", 100 + 10 * s + t, 1)
            p.import_device(f=one, first_tracer=t)
        plans.append(p)
    M.fill_synthetic(one, "f", 99, 1)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows)}

    # the check first: one call per mode against torch.cumsum on the exported copies
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    fx = torch.empty(M.shapes(ncrms, nx, nz, T)["f"], dtype=tdt, device=dev)
    for name, mode in MODES.items():
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        p = wgt.double().unsqueeze(-2) * fx[0, :, 3:nx + 3, :].double()          # (nzm, nx, ncrms)
        if mode & M.COLUMN_SCAN_DOWN:
            p = p.flip(0)
        o = p.cumsum(0)
        tot = o[-1].clone()
        if mode & M.COLUMN_SCAN_EXCLUSIVE:
            o = o - p
        if mode & M.COLUMN_SCAN_DOWN:
            o = o.flip(0)
        plans[0].column_scan(0, 1, wgt, total, mode)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        scale = float(p.abs().sum(0).max()) + 1.0
        err = float((fx[1, :, 3:nx + 3, :].double() - o).abs().max() / scale)
        assert err < 4 * nzm * eps, (tag, name, err)
        errt = float((total.double() - tot).abs().max() / scale)
        assert errt < 4 * nzm * eps, (tag, name, errt)
        del p, o, tot
    del fx
    torch.cuda.empty_cache()

    def restore():
        for q in plans:                 # the in-place tracer back to a field of order one (untimed)
            q.import_device(f=one, first_tracer=2)

    lo, di, up = (rnd(M.vsolve_shapes(ncrms, nz)[k], *r) for k, r in (("lo", (-0.4, 0.0)), ("di", (1.0, 1.8)), ("up", (-0.4, 0.0))))
    path = torch.empty(M.column_path_shapes(ncrms, nx)["path"], dtype=tdt, device=dev)
    d1 = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
    runs = {}
    for name, mode in MODES.items():
        runs[f"scan_{name}"] = (lambda i, mode=mode: plans[i % n].column_scan(0, 1, wgt, total, mode), None)
        runs[f"scan_{name}_inplace"] = (lambda i, mode=mode: plans[i % n].column_scan(2, 2, wgt, total, mode), restore)
    runs["scan_up_nowgt"] = (lambda i: plans[i % n].column_scan(0, 1), None)
    runs["vsolve"] = (lambda i: plans[i % n].vsolve(lo, di, up, first_tracer=1, ntracers=1), None)
    runs["column_path"] = (lambda i: plans[i % n].column_path(path, first_tracer=0, ntracers=1), None)
    runs["level_add"] = (lambda i: plans[i % n].level_add(d1, first_tracer=1), None)

    def round_trip(i):
        plans[i % n].export_device(f=one, first_tracer=0)
        plans[i % n].import_device(f=one, first_tracer=1)
    runs["round_trip"] = (round_trip, None)
    for k, (fn, between) in runs.items():
        if a.only and k != a.only:
            continue
        # (the in-place scans grow the field by up to nzm per call: one call per plan and round)
        st = n if between else steps
        res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"] = timed(fn, st, between)
        res[k + "_spread"] = (res[k + "_ms_max"] - res[k + "_ms_min"]) / res[k + "_ms"]
        print(f"{tag:9s} {k:24s} {res[k + '_ms']:.4f} ms ({res[k + '_ms_min']:.4f} .. {res[k + '_ms_max']:.4f})", flush=True)
    if not a.only:
        alg = col * nx * 2
        res["algorithmic_bytes"] = alg
        for name in MODES:
            res[f"scan_{name}_tbs"] = alg / res[f"scan_{name}_ms"] / 1e9
        for y in ("vsolve", "column_path", "level_add", "round_trip"):
            res[f"ratio_scan_up_over_{y}"] = res["scan_up_ms"] / res[y + "_ms"]
            res[f"ratio_scan_up_inplace_over_{y}"] = res["scan_up_inplace_ms"] / res[y + "_ms"]
        res["ratio_down_over_up"] = res["scan_down_ms"] / res["scan_up_ms"]
        res["down_vs_up_resolved"] = abs(res["scan_down_ms"] - res["scan_up_ms"]) > max(
            res["scan_down_ms_max"] - res["scan_down_ms_min"], res["scan_up_ms_max"] - res["scan_up_ms_min"])
        print(f"{tag:9s} scan up {res['scan_up_ms']:.4f} ms ({res['scan_up_tbs']:.2f} TB/s)  x vsolve {res['ratio_scan_up_over_vsolve']:.3f}  "
              f"x column_path {res['ratio_scan_up_over_column_path']:.3f}  x level_add {res['ratio_scan_up_over_level_add']:.3f}  "
              f"x export + import {res['ratio_scan_up_over_round_trip']:.3f}  down / up {res['ratio_down_over_up']:.3f} "
              f"({'resolved' if res['down_vs_up_resolved'] else 'unresolved'})", flush=True)
    for p in plans:
        p.close()
    del plans
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
prec = [("f64", torch.float64, 8)] + ([] if a.no_f32 else [("f32", torch.float32, 4)])
cases = [(t, tuple(a.shape), tdt, eb, a.sets, False) for t, tdt, eb in prec]
if not a.no_tall:
    cases += [(t + "_tall", tuple(a.tall_shape), tdt, eb, a.sets, True) for t, tdt, eb in prec]
for tag, shape, tdt, eb, sets, tall in cases:
    measure(tag, shape, tdt, eb, sets, a.steps, tall)
M.set_tall_columns(0)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
