#!/usr/bin/env python3
"""Time of the linear combinations of the tracers of a resident plan (include/mpdata_hip.h 3z), cold, at ncrms=65536 nx=32
nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), nine tracers, fp64 and fp32: consecutive calls go to different
plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch events around
a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped falling, i.e. two
consecutive batches agree within 3 %; then the median, the minimum and the maximum of five batches):
  combine_N      : Plan.combine of N = 0, 1, 2, 4, 8 distinct sources (tracers 0 .. N-1) into tracer 8, the whole plan, with
                   coef, c0 and sum
  combine_N_bare : the same without coef, c0 (N > 0) and sum -- N = 1: the copy
  combine_2_inplace : dst among the two sources
  combine_8_block   : 8 sources on a block of 64 instances
and the yardsticks in the same process, all of them calls that exist without 3z:
  round_trip_N   : Plan.export_device of the N source tracers + Plan.import_device of dst -- the route a caller had before
                   the call existed, without the caller's own kernel
  level_add      : one Plan.level_add of one tracer (against N = 1: the same interior bytes, and the halo columns on top)
  convert        : Plan.convert with r alone (against N = 2: two reads and TWO writes, one write more)
and from them the ratios and TB/s against the algorithmic bytes: the interior of N tracers read and one written, (N + 1) nx
nzm ncrms reals.  The result of one call per N is checked against torch on the exported copies (to rounding: torch may
contract).  The columns-in-flight candidates of a class (MPDATA_COMBINE_NB_LO / _MID / _HI, MPDATA_COMBINE_HI_SERIAL of
csrc/mpdata_combine.h) are compile-time: this tool is run once per library (MPDATA_HIP_LIB names the library, --tag names
the run) and adds its run to the JSON under that tag.  Needs no oracle and no reference tree.
usage: python tools/combine_bench.py [--steps K] [--sets N] [--json PATH] [--tag NAME] [--nsrc 0 1 2 4 8] [--no-f32] [--no-tall]
                                     [--no-yardsticks]"""
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
ap.add_argument("--block", type=int, default=64, help="instances of the block case")
ap.add_argument("--nsrc", type=int, nargs="+", default=[0, 1, 2, 4, 8])
ap.add_argument("--json", default=None)
ap.add_argument("--tag", default="kept", help="a name for the run in the JSON (the library's columns in flight)")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--no-yardsticks", action="store_true", help="the combine calls alone (a candidate library)")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0), "library": os.path.basename(M.lib_path())}
T, DST = 9, 8


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps):
    """-> (median, min, max) of five batches behind the wake-up"""
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = loop_ms(fn, steps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    t = [loop_ms(fn, steps) for _ in range(5)]
    return statistics.median(t), min(t), max(t)


def measure(tag, shape, tdt, eb, sets, steps, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    csh = {N: M.combine_shapes(ncrms, nx, nz, N) for N in a.nsrc}
    coef = {N: rnd(csh[N]["coef"], -1.0, 1.0) for N in a.nsrc if N}
    c0 = rnd((nzm, ncrms), -0.5, 0.5)
    ssum = torch.empty((nzm, ncrms), dtype=tdt, device=dev)
    nb = min(a.block, ncrms)
    coef_b, c0_b = rnd(M.combine_shapes(nb, nx, nz, 8)["coef"], -1.0, 1.0), rnd((nzm, nb), -0.5, 0.5)
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
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows)}

    # the check first: one call per N with everything, clipped, against torch on the exported copies
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    fx = torch.empty(M.shapes(ncrms, nx, nz, T)["f"], dtype=tdt, device=dev)
    for N in a.nsrc:
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        f0 = fx[:, :, 3:nx + 3, :].double()
        plans[0].combine(DST, range(N), coef.get(N), c0, M.COMBINE_CLIP, ssum)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        v = c0.double().unsqueeze(-2).expand(nzm, nx, ncrms).clone()
        for j in range(N):
            v += coef[N][j].double().unsqueeze(-2) * f0[j]
        v.clamp_(min=0)
        scale = float(f0.abs().max()) * max(N, 1) + 1.0
        err = float((fx[DST, :, 3:nx + 3, :].double() - v).abs().max() / scale)
        assert err < 4 * (N + 1) * eps, (tag, N, err)
        errs = float((ssum.double() - v.sum(dim=-2)).abs().max() / scale)
        assert errs < nx * nx * (N + 1) * eps, (tag, N, errs)   # (nx adds, each partial sum below nx * scale)
        assert torch.equal(fx[:DST, :, 3:nx + 3, :].double(), f0[:DST]), "a source changed"
        assert float(v.max()) > 0 and float((v == 0).double().mean()) > 0.01
        del f0, v
    del fx
    torch.cuda.empty_cache()

    runs = {}
    for N in a.nsrc:
        runs[f"combine_{N}"] = lambda i, N=N: plans[i % n].combine(DST, range(N), coef.get(N), c0, 0, ssum)
        runs[f"combine_{N}_bare"] = lambda i, N=N: plans[i % n].combine(DST, range(N), None, c0 if N == 0 else None)
    if 2 in a.nsrc:
        runs["combine_2_inplace"] = lambda i: plans[i % n].combine(1, (0, 1), coef[2], c0, 0, ssum)
    if 8 in a.nsrc:
        runs["combine_8_block"] = lambda i: plans[i % n].combine(DST, range(8), coef_b, c0_b, sl0=(ncrms - nb) // 2, n=nb)
    if not a.no_yardsticks:
        fxs = {N: torch.empty(M.shapes(ncrms, nx, nz, N)["f"] if N > 1 else one.shape, dtype=tdt, device=dev) for N in a.nsrc if N}

        def round_trip(i, N):
            if N:
                plans[i % n].export_device(f=fxs[N], first_tracer=0)
            plans[i % n].import_device(f=one, first_tracer=DST)
        for N in a.nsrc:
            runs[f"round_trip_{N}"] = lambda i, N=N: round_trip(i, N)
        d1 = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
        r = rnd((nzm, ncrms), 0.005, 0.02)
        runs["level_add"] = lambda i: plans[i % n].level_add(d1, first_tracer=DST)
        runs["convert"] = lambda i: plans[i % n].convert(0, 1, r)
    for k, fn in runs.items():
        res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"] = timed(fn, steps)
    for N in a.nsrc:
        alg = col * nx * (N + 1)
        res[f"algorithmic_bytes_{N}"] = alg
        for k in (f"combine_{N}", f"combine_{N}_bare"):
            res[k + "_tbs"] = alg / res[k + "_ms"] / 1e9
        if not a.no_yardsticks:
            res[f"round_trip_{N}_bytes"] = col * (nx + 6) * (2 * N + 2)
            res[f"ratio_combine_{N}_over_round_trip"] = res[f"combine_{N}_ms"] / res[f"round_trip_{N}_ms"]
        line = f"{tag:9s} nsrc {N}: {res[f'combine_{N}_ms']:.4f} ms ({res[f'combine_{N}_ms_min']:.4f} .. {res[f'combine_{N}_ms_max']:.4f}; " \
               f"{res[f'combine_{N}_tbs']:.2f} TB/s)  bare {res[f'combine_{N}_bare_ms']:.4f} ({res[f'combine_{N}_bare_tbs']:.2f} TB/s)"
        if not a.no_yardsticks:
            line += f"  export of {N} + import of 1: {res[f'round_trip_{N}_ms']:.4f}  ratio {res[f'ratio_combine_{N}_over_round_trip']:.3f}"
        print(line, flush=True)
    if not a.no_yardsticks:
        if 1 in a.nsrc:
            res["ratio_combine_1_over_level_add"] = res["combine_1_ms"] / res["level_add_ms"]
            res["ratio_combine_1_bare_over_level_add"] = res["combine_1_bare_ms"] / res["level_add_ms"]
        if 2 in a.nsrc:
            res["ratio_combine_2_over_convert"] = res["combine_2_ms"] / res["convert_ms"]
        print(f"{tag:9s} level_add {res['level_add_ms']:.4f} ms  convert (r alone) {res['convert_ms']:.4f} ms  in place "
              f"{res.get('combine_2_inplace_ms', float('nan')):.4f}  block of {nb}, 8 sources {res.get('combine_8_block_ms', float('nan')):.4f}",
              flush=True)
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
print(json.dumps({a.tag: out}))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    allruns = json.load(open(a.json)) if os.path.exists(a.json) else {}
    allruns[a.tag] = out
    with open(a.json, "w") as fh:
        json.dump(allruns, fh, indent=1)
