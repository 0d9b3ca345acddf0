#!/usr/bin/env python3
"""Time of the first-order conversion between two tracers of a resident plan (include/mpdata_hip.h 3t), cold, at
ncrms=65536 nx=32 nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), two tracers, fp64 and fp32: consecutive calls go
to different plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch
events around a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped
falling, i.e. two consecutive batches agree within 3 %; then the minimum AND the maximum of three batches, the run-to-run
spread):
  convert_all    : Plan.convert 0 -> 1, the whole plan, with q0, y and dsum; r != 0 on every level (every level is rewritten)
  convert_none   : r alone
  convert_limit  : r alone, mode CONVERT_LIMIT
  convert_back   : r alone, 1 -> 0 (the negative offset between the two streams)
  convert_block  : r alone on a block of 64 instances
and three yardsticks in the same process, all of them calls that exist without 3t:
  round_trip  : (a) Plan.export_device + Plan.import_device of both tracers of f -- the route a caller had before the call
                existed, without the caller's own kernel
  level_add2  : (b) two Plan.level_add calls, one tracer each -- the same interior bytes (and the halo columns on top)
  relax2      : (c) Plan.relax to a target, twice, one tracer each -- the same bytes exactly
and from them the ratios and GB/s against the bytes each call moves: convert 4 nx nzm ncrms reals (the interior of two
tracers read once and written once), relax2 the same, level_add2 4 (nx + 6) columns, the round trip 8 (nx + 6).  The result
of one call is checked against torch on the exported copies (to rounding: torch may contract).  Needs no oracle and no
reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/convert_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall]"""
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
ap.add_argument("--block", type=int, default=64, help="instances of the block case")
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. convert_all")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0)}
T = 2


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


def measure(tag, shape, tdt, eb, sets, steps, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, T)
    csh = M.convert_shapes(ncrms, nx, nz)
    bsh = M.convert_shapes(min(a.block, ncrms), nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    r = rnd(csh["r"], 0.005, 0.02)                         # != 0 on every level: every level is loaded and stored
    rb = rnd(bsh["r"], 0.005, 0.02)
    q0, y = rnd(csh["q0"], 0.3, 0.6), rnd(csh["y"], 0.5, 1.5)
    dsum = torch.empty(csh["dsum"], dtype=tdt, device=dev)
    d1 = torch.zeros(csh["r"], dtype=tdt, device=dev)      # level_add of one tracer
    tgt = rnd(csh["r"], 0.2, 0.8)
    plans = []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        for t in range(T):
            M.fill_synthetic(ftmp[t], "f", 100 + 10 * s + t, 1)
        p.import_device(f=ftmp)
        plans.append(p)
    del ftmp
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances of one tracer
    alg = col * 4 * nx                                   # the interior of two tracers read and written
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows), "algorithmic_bytes": alg,
           "level_add2_bytes": col * 4 * (nx + 6), "relax2_bytes": alg, "round_trip_bytes": col * 8 * (nx + 6)}

    # the check first (the timed calls go on changing the same fields): one call with everything, capped, against torch on
    # the exported copies, with an r that is zero on the lower half of the levels and up to 2 above
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    rr = rnd(csh["r"], 0.25, 2.0)
    rr[:nzm // 2] = 0
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    f0 = fx.clone().double()                              # (T, nzm, nx+6, ncrms)
    plans[0].convert(0, 1, rr, q0, y, M.CONVERT_LIMIT, dsum)
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    src, dst = f0[0, :, 3:nx + 3, :], f0[1, :, 3:nx + 3, :]
    e = (src - q0.double().unsqueeze(-2)).clamp_min(0)
    dd = torch.minimum(rr.double().unsqueeze(-2) * e, src.clamp_min(0))
    want = f0.clone()
    want[0, :, 3:nx + 3, :] = src - dd
    want[1, :, 3:nx + 3, :] = dst + y.double().unsqueeze(-2) * dd
    scale = float(f0.abs().max()) + 1.0
    err = float((fx.double() - want).abs().max() / scale)
    assert err < 8 * eps, (tag, err)
    errs = float((dsum.double() - dd.sum(dim=-2)).abs().max() / scale)
    assert errs < 2 * nx * eps, (tag, errs)
    assert torch.equal(fx[:, :nzm // 2].double(), f0[:, :nzm // 2]), "a level with r == 0 changed"
    assert not torch.equal(fx[0, nzm // 2:, 3:nx + 3].double(), src[nzm // 2:]) and float(dd.max()) > 0
    assert torch.equal(fx[..., :3, :].double(), f0[..., :3, :]) and torch.equal(fx[..., nx + 3:, :].double(), f0[..., nx + 3:, :]), \
        "halo columns changed"
    del f0, want, src, dst, e, dd
    torch.cuda.empty_cache()

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    def level_add2(i):
        plans[i % n].level_add(d1, first_tracer=0)
        plans[i % n].level_add(d1, first_tracer=1)

    def relax2(i):
        plans[i % n].relax(r, tgt, first_tracer=0, ntracers=1)
        plans[i % n].relax(r, tgt, first_tracer=1, ntracers=1)

    nb = min(a.block, ncrms)
    runs = {
        "convert_all": lambda i: plans[i % n].convert(0, 1, r, q0, y, 0, dsum),
        "convert_none": lambda i: plans[i % n].convert(0, 1, r),
        "convert_limit": lambda i: plans[i % n].convert(0, 1, r, mode=M.CONVERT_LIMIT),
        "convert_back": lambda i: plans[i % n].convert(1, 0, r),
        "convert_block": lambda i: plans[i % n].convert(0, 1, rb, sl0=(ncrms - nb) // 2, n=nb),
        "round_trip": round_trip,
        "level_add2": level_add2,
        "relax2": relax2,
    }
    if a.only:
        res[a.only + "_ms"], res[a.only + "_ms_max"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_ms_max"] = timed(fn, steps)
        res["convert_all_ms_again"], _ = timed(runs["convert_all"], steps)
        res["convert_none_ms_again"], _ = timed(runs["convert_none"], steps)
        res["level_add2_ms_again"], _ = timed(runs["level_add2"], steps)
        for c in ("convert_all", "convert_none"):
            for k in ("round_trip", "level_add2", "relax2"):
                res[f"ratio_{c}_over_{k}"] = res[c + "_ms"] / res[k + "_ms"]
            res[c + "_gbs"] = alg / res[c + "_ms"] / 1e6
        for k in ("level_add2", "relax2", "round_trip"):
            res[k + "_gbs"] = res[k + "_bytes"] / res[k + "_ms"] / 1e6
        print(f"{tag:12s}: convert with all {res['convert_all_ms']:.4f} ms (max {res['convert_all_ms_max']:.4f}, again "
              f"{res['convert_all_ms_again']:.4f}; {res['convert_all_gbs']:.0f} GB/s)  r alone {res['convert_none_ms']:.4f} (max "
              f"{res['convert_none_ms_max']:.4f}, again {res['convert_none_ms_again']:.4f}; {res['convert_none_gbs']:.0f} GB/s)  LIMIT "
              f"{res['convert_limit_ms']:.4f}  1 -> 0 {res['convert_back_ms']:.4f}  block of {nb} {res['convert_block_ms']:.4f}  "
              f"(a) export + import of both tracers {res['round_trip_ms']:.4f} ({res['round_trip_gbs']:.0f} GB/s)  (b) two level_add "
              f"{res['level_add2_ms']:.4f} (max {res['level_add2_ms_max']:.4f}, again {res['level_add2_ms_again']:.4f}; "
              f"{res['level_add2_gbs']:.0f} GB/s)  (c) two relax {res['relax2_ms']:.4f} ({res['relax2_gbs']:.0f} GB/s)  all / (a) "
              f"{res['ratio_convert_all_over_round_trip']:.3f}  / (b) {res['ratio_convert_all_over_level_add2']:.3f}  / (c) "
              f"{res['ratio_convert_all_over_relax2']:.3f}  r alone / (a) {res['ratio_convert_none_over_round_trip']:.3f}  / (b) "
              f"{res['ratio_convert_none_over_level_add2']:.3f}  / (c) {res['ratio_convert_none_over_relax2']:.3f}", flush=True)
    for p in plans:
        p.close()
    del plans, fx
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
