#!/usr/bin/env python3
"""Time of the per-cell sources of a resident plan (include/mpdata_hip.h 3p), one tracer, cold, at ncrms=65536 nx=32 nz=28
and at ncrms=4096 nx=32 nz=300 (a windowed plan), fp64 and fp32: consecutive calls go to different plans (field sets)
with their own s, as bench.py runs its steps, so no call finds its f or its s in the Infinity Cache.  Per call (torch
events around a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped
falling, i.e. two consecutive batches agree within 3 %):
  cell_add           : Plan.cell_add, the whole plan, CELL_ADD, dsum = None
  cell_add_dsum      : the same with dsum
  cell_add_clip      : CELL_ADD_CLIP, dsum = None
  cell_add_clip_dsum : CELL_ADD_CLIP with dsum
and three yardsticks in the same process, all of them calls that exist without 3p:
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel
  level_add     : Plan.level_add -- reads and writes every column slot of f, no per-cell field
  sediment      : Plan.sediment, psfc = pflux = None -- the same algorithmic bytes through the same staging, plus a stencil
                  along k, a second barrier per round and an edge load
and from them the ratios and GB/s against the bytes each call moves: cell_add and sediment their algorithmic traffic (the
interior of f read once and written once, s or wp read once: 3 nx nzm ncrms reals), level_add 2 (nx + 6) columns, the round
trip twice that.  The result of one call of each mode is checked against torch on the exported copies (to rounding: torch
may contract).  Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them
all there.
usage: python tools/cell_add_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall]"""
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
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="the plain shape only")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. cell_add")
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
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = loop_ms(fn, steps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return min(loop_ms(fn, steps) for _ in range(3))


def measure(tag, shape, tdt, eb, sets, steps, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, 1)
    csh = M.cell_add_shapes(ncrms, nx, nz)
    ssh = M.sediment_shapes(ncrms, nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    dsum = torch.empty(csh["dsum"], dtype=tdt, device=dev)
    d = torch.zeros((nzm, ncrms), dtype=tdt, device=dev)
    plans, ss, wps = [], [], []
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
        # (small values of both signs: hundreds of timed calls on one field stay finite)
        ss.append(rnd(csh["s"], -0.004, 0.004))
        wps.append(rnd(ssh["wp"], -0.002, 0.008))
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances
    alg = col * 3 * nx                                   # the interior of f read and written, s read
    res = {"shape": [ncrms, nx, nz], "level_windows": int(plans[0].level_windows), "algorithmic_bytes": alg,
           "level_add_bytes": col * 2 * (nx + 6), "round_trip_bytes": col * 4 * (nx + 6)}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on changing the same fields): one call of each mode against torch on the
    # exported copies; s scaled up so that the clip acts on a part of the cells
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    for mode in (M.CELL_ADD, M.CELL_ADD_CLIP):
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        f0 = fx.clone().double()                              # (nzm, nx+6, ncrms); a copy also where fx is float64
        c = -150.0
        plans[0].cell_add(ss[0], c, mode, dsum)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        cf = float(torch.tensor(c, dtype=tdt))
        want = f0.clone()
        want[:, 3:nx + 3] += cf * ss[0].double()
        if mode == M.CELL_ADD_CLIP:
            frac = float((want[:, 3:nx + 3] < 0).double().mean())
            assert 0.02 < frac < 0.98, (tag, frac)
            want[:, 3:nx + 3].clamp_(min=0.0)
        scale = float(f0.abs().max()) + 150.0 * 0.004
        err = float((fx.double() - want).abs().max() / scale)
        assert err < 8 * eps, (tag, mode, err)
        wd = (want[:, 3:nx + 3] - f0[:, 3:nx + 3]).sum(dim=1)
        errd = float((dsum.double() - wd).abs().max() / (nx * scale))
        assert errd < 4 * nx * eps, (tag, mode, errd)
        assert torch.equal(fx[:, :3].double(), f0[:, :3]) and torch.equal(fx[:, nx + 3:].double(), f0[:, nx + 3:]), "halo columns changed"
        del f0, want, wd
    torch.cuda.empty_cache()

    runs = {
        "cell_add": lambda i: plans[i % n].cell_add(ss[i % n], 0.75),
        "cell_add_dsum": lambda i: plans[i % n].cell_add(ss[i % n], 0.75, M.CELL_ADD, dsum),
        "cell_add_clip": lambda i: plans[i % n].cell_add(ss[i % n], 0.75, M.CELL_ADD_CLIP),
        "cell_add_clip_dsum": lambda i: plans[i % n].cell_add(ss[i % n], 0.75, M.CELL_ADD_CLIP, dsum),
        "round_trip": round_trip,
        "level_add": lambda i: plans[i % n].level_add(d),
        "sediment": lambda i: plans[i % n].sediment(wps[i % n]),
    }
    if a.only:
        res[a.only + "_ms"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"] = timed(fn, steps)
        res["cell_add_ms_again"] = timed(runs["cell_add"], steps)
        for k in ("round_trip", "level_add", "sediment"):
            res["ratio_cell_add_over_" + k] = res["cell_add_ms"] / res[k + "_ms"]
        res["ratio_dsum_over_plain"] = res["cell_add_dsum_ms"] / res["cell_add_ms"]
        res["cell_add_gbs"] = alg / res["cell_add_ms"] / 1e6
        res["sediment_gbs"] = alg / res["sediment_ms"] / 1e6
        res["level_add_gbs"] = res["level_add_bytes"] / res["level_add_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        print(f"{tag:12s}: cell_add {res['cell_add_ms']:.4f} ms ({res['cell_add_gbs']:.0f} GB/s; again {res['cell_add_ms_again']:.4f})  "
              f"with dsum {res['cell_add_dsum_ms']:.4f}  clip {res['cell_add_clip_ms']:.4f}  clip with dsum "
              f"{res['cell_add_clip_dsum_ms']:.4f}  export + import of f {res['round_trip_ms']:.4f} ({res['round_trip_gbs']:.0f} GB/s)  "
              f"level_add {res['level_add_ms']:.4f} ({res['level_add_gbs']:.0f} GB/s)  sediment {res['sediment_ms']:.4f} "
              f"({res['sediment_gbs']:.0f} GB/s)  cell_add / round trip {res['ratio_cell_add_over_round_trip']:.3f}  / level_add "
              f"{res['ratio_cell_add_over_level_add']:.3f}  / sediment {res['ratio_cell_add_over_sediment']:.3f}", flush=True)
    for p in plans:
        p.close()
    del plans, ss, wps, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
cases = [("f64", tuple(a.shape), torch.float64, 8, False)]
if not a.no_f32:
    cases.append(("f32", tuple(a.shape), torch.float32, 4, False))
if not a.no_tall:
    cases.append(("f64_tall", tuple(a.tall_shape), torch.float64, 8, True))
    if not a.no_f32:
        cases.append(("f32_tall", tuple(a.tall_shape), torch.float32, 4, True))
for tag, shape, tdt, eb, tall in cases:
    measure(tag, shape, tdt, eb, a.sets, a.steps, tall)
M.set_tall_columns(0)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
