#!/usr/bin/env python3
"""Time of the relaxation of a resident plan's tracers to a level profile (include/mpdata_hip.h 3r), cold, at ncrms=65536
nx=32 nz=28 with one tracer and with 25, and at ncrms=4096 nx=32 nz=300 (a windowed plan), fp64 and fp32: consecutive
calls go to different plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache (the
25-tracer plans are one set: a call moves more bytes than any cache holds).  Per call (torch events around a loop of calls
on the plans' stream, after a wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive
batches agree within 3 %; then the minimum AND the maximum of three batches, the run-to-run spread):
  relax_mean        : Plan.relax, the whole plan, no target, mean = None; c != 0 on every level (every level is rewritten)
  relax_mean_out    : the same with mean
  relax_target      : with a target, mean = None
  relax_target_out  : with a target and mean
and three yardsticks in the same process, all of them calls that exist without 3r:
  round_trip  : (a) Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                without the caller's own kernel
  stats_add   : (b) Plan.level_stats (sum only) + Plan.level_add -- the same bytes from HBM plus one more read of f
  level_add   : (c) Plan.level_add alone -- one read and one write of f, the floor
and from them the ratios and GB/s against the bytes each call moves: relax 2 nx nzm ncrms reals (the interior of f read
once and written once; the second read of mean mode is not counted), level_add 2 (nx + 6) columns, stats_add that plus nx
columns, the round trip 4 (nx + 6).  The result of one call of each mode is checked against torch on the exported copies
(to rounding: torch may contract and sums in another order).  Needs no oracle and no reference tree.  Prints one line per
measurement and, with --json PATH, writes them all there.
usage: python tools/relax_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--no-tracers]"""
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
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tracers", type=int, default=25, help="tracers of the many-tracer case")
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--no-tracers", action="store_true", help="no many-tracer case")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. relax_mean")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0)}


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps):
    """-> (min, max) of three batches behind the wake-up"""
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = loop_ms(fn, steps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    t = [loop_ms(fn, steps) for _ in range(3)]
    return min(t), max(t)


def measure(tag, shape, T, tdt, eb, sets, steps, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, T)
    rsh = M.relax_shapes(ncrms, nx, nz, T if T > 1 else None)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    mean = torch.empty(rsh["mean"], dtype=tdt, device=dev)
    ssum = torch.empty(rsh["mean"], dtype=tdt, device=dev)
    target = rnd(rsh["target"], 0.2, 0.8)
    c = rnd(rsh["c"], 0.005, 0.02)                        # != 0 on every level: every level is loaded and stored
    d = torch.zeros(rsh["mean"], dtype=tdt, device=dev)
    plans = []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp)
        plans.append(p)
    del ftmp
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb * T                    # bytes of one column of all instances and tracers
    alg = col * 2 * nx                                   # the interior of f read and written
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows), "algorithmic_bytes": alg,
           "level_add_bytes": col * 2 * (nx + 6), "stats_add_bytes": col * (3 * nx + 12), "round_trip_bytes": col * 4 * (nx + 6)}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    def stats_add(i):
        plans[i % n].level_stats(sum=ssum)
        plans[i % n].level_add(d)

    # the check first (the timed calls go on changing the same fields): one call of each mode against torch on the
    # exported copies, with a c that is zero on the lower half of the levels and large above
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    cc = rnd(rsh["c"], 0.25, 1.0)
    cc[:nzm // 2] = 0
    for tgt in (None, target):
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        f0 = fx.clone().double()                              # ([T,] nzm, nx+6, ncrms); a copy also where fx is float64
        plans[0].relax(cc, tgt, mean)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        fi = f0[..., 3:nx + 3, :]
        mw = fi.sum(dim=-2) / nx if tgt is None else tgt.double()
        want = f0.clone()
        want[..., 3:nx + 3, :] = fi - cc.double().unsqueeze(-2) * (fi - mw.unsqueeze(-2))
        scale = float(f0.abs().max()) + 1.0
        errm = float((mean.double() - mw).abs().max() / scale)
        assert errm < 2 * nx * eps, (tag, tgt is None, errm)
        err = float((fx.double() - want).abs().max() / scale)
        assert err < (2 * nx + 8) * eps, (tag, tgt is None, err)
        assert torch.equal(fx[..., :nzm // 2, :, :].double(), f0[..., :nzm // 2, :, :]), "a level with c == 0 changed"
        assert not torch.equal(fx[..., nzm // 2:, 3:nx + 3, :].double(), fi[..., nzm // 2:, :, :])
        assert torch.equal(fx[..., :3, :].double(), f0[..., :3, :]) and torch.equal(fx[..., nx + 3:, :].double(), f0[..., nx + 3:, :]), \
            "halo columns changed"
        del f0, want, fi, mw
    torch.cuda.empty_cache()

    runs = {
        "relax_mean": lambda i: plans[i % n].relax(c, ntracers=T),
        "relax_mean_out": lambda i: plans[i % n].relax(c, None, mean),
        "relax_target": lambda i: plans[i % n].relax(c, target, ntracers=T),
        "relax_target_out": lambda i: plans[i % n].relax(c, target, mean),
        "round_trip": round_trip,
        "stats_add": stats_add,
        "level_add": lambda i: plans[i % n].level_add(d),
    }
    if a.only:
        res[a.only + "_ms"], res[a.only + "_ms_max"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_ms_max"] = timed(fn, steps)
        res["relax_mean_ms_again"], _ = timed(runs["relax_mean"], steps)
        res["relax_target_ms_again"], _ = timed(runs["relax_target"], steps)
        res["level_add_ms_again"], _ = timed(runs["level_add"], steps)
        for r in ("relax_mean", "relax_target"):
            for k in ("round_trip", "stats_add", "level_add"):
                res[f"ratio_{r}_over_{k}"] = res[r + "_ms"] / res[k + "_ms"]
            res[r + "_gbs"] = alg / res[r + "_ms"] / 1e6
        res["level_add_gbs"] = res["level_add_bytes"] / res["level_add_ms"] / 1e6
        res["stats_add_gbs"] = res["stats_add_bytes"] / res["stats_add_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        print(f"{tag:12s}: relax to the mean {res['relax_mean_ms']:.4f} ms (max {res['relax_mean_ms_max']:.4f}, again "
              f"{res['relax_mean_ms_again']:.4f}; {res['relax_mean_gbs']:.0f} GB/s)  with mean {res['relax_mean_out_ms']:.4f}  "
              f"to a target {res['relax_target_ms']:.4f} (max {res['relax_target_ms_max']:.4f}, again {res['relax_target_ms_again']:.4f}; "
              f"{res['relax_target_gbs']:.0f} GB/s)  with mean {res['relax_target_out_ms']:.4f}  (a) export + import of f "
              f"{res['round_trip_ms']:.4f} ({res['round_trip_gbs']:.0f} GB/s)  (b) level_stats + level_add {res['stats_add_ms']:.4f} "
              f"({res['stats_add_gbs']:.0f} GB/s)  (c) level_add {res['level_add_ms']:.4f} (max {res['level_add_ms_max']:.4f}, again "
              f"{res['level_add_ms_again']:.4f}; {res['level_add_gbs']:.0f} GB/s)  mean / (a) {res['ratio_relax_mean_over_round_trip']:.3f}  "
              f"/ (b) {res['ratio_relax_mean_over_stats_add']:.3f}  / (c) {res['ratio_relax_mean_over_level_add']:.3f}  target / (a) "
              f"{res['ratio_relax_target_over_round_trip']:.3f}  / (b) {res['ratio_relax_target_over_stats_add']:.3f}  / (c) "
              f"{res['ratio_relax_target_over_level_add']:.3f}", flush=True)
    for p in plans:
        p.close()
    del plans, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
prec = [("f64", torch.float64, 8)] + ([] if a.no_f32 else [("f32", torch.float32, 4)])
cases = [(t, tuple(a.shape), 1, tdt, eb, a.sets, False) for t, tdt, eb in prec]
if not a.no_tracers:
    cases += [(f"{t}_{a.tracers}tr", tuple(a.shape), a.tracers, tdt, eb, 1, False) for t, tdt, eb in prec]
if not a.no_tall:
    cases += [(t + "_tall", tuple(a.tall_shape), 1, tdt, eb, a.sets, True) for t, tdt, eb in prec]
for tag, shape, T, tdt, eb, sets, tall in cases:
    measure(tag, shape, T, tdt, eb, sets, a.steps if T == 1 else max(3, a.steps // 5), tall)
M.set_tall_columns(0)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
