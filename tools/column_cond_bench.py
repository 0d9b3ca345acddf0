#!/usr/bin/env python3
"""Time of the per-column conditional level counts, tops and paths of a resident plan's tracers (include/mpdata_hip.h 3w),
cold, at ncrms=65536 nx=32 nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), plans of nine tracers (the condition
and eight value tracers), fp64 and fp32: consecutive calls go to different plans (field sets), as bench.py runs its steps,
so no call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a
wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %; then the
minimum AND the maximum of three batches, the run-to-run spread), with tc = 0 and the value tracers 1 .. T:
  kc                      : kcnt and cover alone, lo and hi (only tc is staged)
  kall                    : kcnt, kbot, ktop and cover
  cp1, cp3, cp8           : cpath of T = 1, 3, 8 value tracers, lo and hi
  cp3_all                 : all six outputs with three value tracers
  cp3_hi                  : cp3 under hi alone
  cp3_block               : cp3 on a block of 64 instances
and two yardsticks per T in the same process on the same plans, calls that exist without 3w:
  exportT  : (a) Plan.export_device of the T + 1 tracers -- the route the call replaces, without the caller's own kernel
  pathT    : (b) Plan.column_path of T + 1 tracers -- the same bytes through the same staging
and from them the ratios and GB/s against the algorithmic bytes: (T + 1) nx nzm ncrms reals (the interior of the T + 1
tracers read once).  The result of one call is checked against torch on an exported copy (the counts and the levels
exactly, the paths to rounding: torch sums in another order).  Needs no oracle and no reference tree.  Prints one line per
measurement and, with --json PATH, writes them all there.
usage: python tools/column_cond_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--label TEXT]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--block", type=int, default=64, help="instances of the block case")
ap.add_argument("--json", default=None)
ap.add_argument("--label", default="default", help="which build of the library this is")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. cp3")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "label": a.label, "library": os.path.basename(M.lib_path()),
       "device": torch.cuda.get_device_name(0)}
TP = 9                                                  # tracers of a plan
TS = (1, 3, 8)


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
    nb = min(a.block, ncrms)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    # the synthetic f lies in [0, 1): about four levels in ten are in
    lo, hi = rnd((nzm, ncrms), 0.2, 0.4), rnd((nzm, ncrms), 0.6, 0.8)
    lob, hib = lo[:, :nb].contiguous(), hi[:, :nb].contiguous()
    new = lambda *sh: torch.empty(sh, dtype=tdt, device=dev)
    kcnt, kbot, ktop, cover = new(nx, ncrms), new(nx, ncrms), new(nx, ncrms), new(ncrms)
    cpath = {T: new(T, nx, ncrms) for T in TS}
    mass3 = new(3, ncrms)
    cpathb = new(3, nx, nb)
    path = new(TP, nx, ncrms)
    plans = []
    ftmp = torch.empty(M.shapes(ncrms, nx, nz, 1)["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, TP, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        for t in range(TP):
            M.fill_synthetic(ftmp, "f", 100 + 10 * s + t, 1)
            p.import_device(f=ftmp, first_tracer=t)
        for nm in ("rho", "adz"):
            x = torch.empty(M.shapes(ncrms, nx, nz, 1)[nm], dtype=tdt, device=dev)
            M.fill_synthetic(x, nm, 100 + s, 1)
            p.import_device(**{nm: x})
            del x
        plans.append(p)
    del ftmp
    fx = torch.empty(M.shapes(ncrms, nx, nz, TP)["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    one = float(nx) * nzm * ncrms * eb                   # the interior of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": TP, "level_windows": int(plans[0].level_windows), "tracer_bytes": one}

    # the check first: the counts, the levels and the paths of three value tracers against torch on an exported copy; the
    # weights are taken from column_path with every level of a one-hot field ... simpler: against column_path under hi = +inf
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    plans[0].export_device(f=fx[:4])
    plans[0].column_cond(0, lo, hi, kcnt, kbot, ktop, cpath[3], cover, mass3, 1)
    torch.cuda.synchronize()
    c = fx[0, :, 3:nx + 3, :]                           # (nzm, nx, ncrms)
    inn = (c > lo.unsqueeze(1)) & (c <= hi.unsqueeze(1))
    lev = torch.arange(1, nzm + 1, device=dev, dtype=torch.float64).view(nzm, 1, 1)
    assert torch.equal(kcnt.double(), inn.sum(dim=0).double()), tag
    assert torch.equal(ktop.double(), (inn * lev).amax(dim=0)), tag
    assert torch.equal(kbot.double(), torch.where(inn, lev, torch.full_like(lev, 1e9)).amin(dim=0).where(inn.any(dim=0), torch.zeros((), dtype=torch.float64, device=dev))), tag
    assert torch.equal(cover.double(), (kcnt > 0).sum(dim=0).double()), tag
    frac = float(inn.double().mean())
    assert 0.02 < frac < 0.98, (tag, frac)
    # every level in: the bits of column_path
    inf = torch.full((nzm, ncrms), float("inf"), dtype=tdt, device=dev)
    chk = new(3, nx, ncrms)
    plans[0].column_cond(0, None, inf, None, None, None, chk, None, None, 1)
    plans[0].column_path(path[:3], None, 0, ncrms, 1, 3)
    torch.cuda.synchronize()
    assert torch.equal(chk.view(torch.uint8), path[:3].view(torch.uint8)), tag
    assert float((mass3.double() - cpath[3].double().sum(dim=1)).abs().max()) <= 4 * nx * eps * float(cpath[3].abs().sum(dim=1).max()), tag
    res["share_in"] = frac
    del c, inn, lev, inf, chk
    torch.cuda.empty_cache()

    runs = {
        "kc": lambda i: plans[i % n].column_cond(0, lo, hi, kcnt, None, None, None, cover),
        "kall": lambda i: plans[i % n].column_cond(0, lo, hi, kcnt, kbot, ktop, None, cover),
        "cp1": lambda i: plans[i % n].column_cond(0, lo, hi, None, None, None, cpath[1], None, None, 1),
        "cp3": lambda i: plans[i % n].column_cond(0, lo, hi, None, None, None, cpath[3], None, None, 1),
        "cp8": lambda i: plans[i % n].column_cond(0, lo, hi, None, None, None, cpath[8], None, None, 1),
        "cp3_all": lambda i: plans[i % n].column_cond(0, lo, hi, kcnt, kbot, ktop, cpath[3], cover, mass3, 1),
        "cp3_hi": lambda i: plans[i % n].column_cond(0, None, hi, None, None, None, cpath[3], None, None, 1),
        "cp3_block": lambda i: plans[i % n].column_cond(0, lob, hib, None, None, None, cpathb, None, None, 1, (ncrms - nb) // 2, nb),
    }
    for T in (0,) + TS:
        runs[f"export{T}"] = lambda i, T=T: plans[i % n].export_device(f=fx[:T + 1] if T else fx[0])
        runs[f"path{T}"] = lambda i, T=T: plans[i % n].column_path(path[:T + 1], None, 0, ncrms, 0, T + 1)
    # the algorithmic bytes: the interior of the tracers the call needs, read once
    ntr = {"kc": 1, "kall": 1, "cp1": 2, "cp3": 4, "cp8": 9, "cp3_all": 4, "cp3_hi": 4}
    base = {"kc": 0, "kall": 0, "cp1": 1, "cp3": 3, "cp8": 8, "cp3_all": 3, "cp3_hi": 3}
    if a.only:
        res[a.only + "_ms"], res[a.only + "_ms_max"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_ms_max"] = timed(fn, steps)
        for k in ("kc", "cp3", "path3"):
            res[k + "_ms_again"], _ = timed(runs[k], steps)
        for k, t in ntr.items():
            res[k + "_gbs"] = t * one / res[k + "_ms"] / 1e6
        for k, T in base.items():
            res[f"ratio_{k}_over_export"] = res[k + "_ms"] / res[f"export{T}_ms"]
            res[f"ratio_{k}_over_path"] = res[k + "_ms"] / res[f"path{T}_ms"]
        ms = lambda k: f"{res[k + '_ms']:.4f}"
        print(f"{tag:12s} [{a.label}]: share in {frac:.2f}  kc {ms('kc')} ms ({res['kc_gbs']:.0f} GB/s; / (a) export {ms('export0')}: "
              f"{res['ratio_kc_over_export']:.3f}, / (b) path {ms('path0')}: {res['ratio_kc_over_path']:.3f}; with kbot, ktop {ms('kall')})  "
              + "  ".join(f"cp{T} {ms(f'cp{T}')} ({res[f'cp{T}_gbs']:.0f} GB/s; / (a) export {ms(f'export{T}')}: "
                          f"{res[f'ratio_cp{T}_over_export']:.3f}, / (b) path {ms(f'path{T}')}: {res[f'ratio_cp{T}_over_path']:.3f})"
                          for T in TS)
              + f"  |  cp3 max {res['cp3_ms_max']:.4f} again {res['cp3_ms_again']:.4f}  hi alone {ms('cp3_hi')}  all six {ms('cp3_all')}  "
              f"block of {nb} {ms('cp3_block')}", flush=True)
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
