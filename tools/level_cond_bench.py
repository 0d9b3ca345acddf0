#!/usr/bin/env python3
"""Time of the per-level conditional counts and sums of a resident plan's tracers (include/mpdata_hip.h 3v), cold, at
ncrms=65536 nx=32 nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), plans of nine tracers (the condition and eight
value tracers), fp64 and fp32: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no call
finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans' stream, after a wake-up:
batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree within 3 %; then the minimum
AND the maximum of three batches, the run-to-run spread), with tc = 0 and the value tracers 1 .. T:
  cnt, cnt_lo             : cnt alone, under lo and hi / under lo alone
  cs1, cs2, cs3, cs8      : cnt and csum of T = 1, 2, 3, 8 value tracers, lo and hi
  cs3_lo                  : cs3 under lo alone
  cs3_in, cs3_neg         : three value tracers 0 .. 2 (tc among them: its walk is the first one) / tc = 8 above them (negative
                            offsets)
  cs3x1                   : the three value tracers as three calls of one tracer each -- the traffic of a tracer axis on
                            the grid (the condition read once per tracer), plus two launches
  cs3_block               : cs3 on a block of 64 instances
and two yardsticks per T in the same process, calls that exist without 3v:
  exportT  : (a) Plan.export_device of the T + 1 tracers -- the route a caller had before the call existed, without the
             caller's own kernel
  statsT   : (b) T + 1 Plan.level_stats calls (sum), one tracer each -- the same bytes read once
and from them the ratios and GB/s against the algorithmic bytes: (T + 1) nx nzm ncrms reals (the interior of the T + 1
tracers read once).  The MASK form against the RE-READ form: run the tool once more on a library whose
mpdata_level_cond.hip was compiled with -DMPDATA_LEVEL_COND_MASK_NX=0 (MPDATA_HIP_LIB names it); --label tags the output.
The result of one call is checked against torch on an exported copy (the count exactly, the sums to rounding: torch sums in
another order).  Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them
all there.
usage: python tools/level_cond_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--label TEXT]"""
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
ap.add_argument("--label", default="default", help="which build of the library this is (mask / re-read)")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. cs3")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "label": a.label, "library": os.path.basename(M.lib_path()),
       "device": torch.cuda.get_device_name(0)}
TP = 9                                                  # tracers of a plan
TS = (1, 2, 3, 8)


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
    # the synthetic f lies in [0, 1): a third of the columns are in
    lo, hi = rnd((nzm, ncrms), 0.2, 0.4), rnd((nzm, ncrms), 0.6, 0.8)
    lob, hib = lo[:, :nb].contiguous(), hi[:, :nb].contiguous()
    cnt = torch.empty((nzm, ncrms), dtype=tdt, device=dev)
    csum = {T: torch.empty((T, nzm, ncrms), dtype=tdt, device=dev) for T in TS}
    cntb, csumb = torch.empty((nzm, nb), dtype=tdt, device=dev), torch.empty((3, nzm, nb), dtype=tdt, device=dev)
    ssum = torch.empty((nzm, ncrms), dtype=tdt, device=dev)
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
        plans.append(p)
    del ftmp
    fx = torch.empty(M.shapes(ncrms, nx, nz, TP)["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    one = float(nx) * nzm * ncrms * eb                   # the interior of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": TP, "level_windows": int(plans[0].level_windows), "tracer_bytes": one}

    # the check first: cnt and csum of three value tracers against torch on an exported copy
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    plans[0].export_device(f=fx[:4])
    plans[0].level_cond(0, lo, hi, cnt, csum[3], 1)
    torch.cuda.synchronize()
    c = fx[0, :, 3:nx + 3, :]                           # (nzm, nx, ncrms)
    inn = (c > lo.unsqueeze(1)) & (c <= hi.unsqueeze(1))
    assert torch.equal(cnt.double(), inn.sum(dim=1).double()), tag
    frac = float(inn.double().mean())
    assert 0.02 < frac < 0.98, (tag, frac)
    for jt in range(3):
        want = torch.where(inn, fx[1 + jt, :, 3:nx + 3, :].double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(dim=1)
        err = float((csum[3][jt].double() - want).abs().max())
        assert err < 4 * nx * nx * eps, (tag, jt, err)
    res["share_in"] = frac
    del c, inn, want
    torch.cuda.empty_cache()

    def stats(T):
        def f(i):
            for t in range(T + 1):
                plans[i % n].level_stats(sum=ssum, first_tracer=t)
        return f

    def cs3x1(i):
        for t in range(3):
            plans[i % n].level_cond(0, lo, hi, cnt if t == 0 else None, csum[3][t:t + 1], 1 + t)

    runs = {
        "cnt": lambda i: plans[i % n].level_cond(0, lo, hi, cnt),
        "cnt_lo": lambda i: plans[i % n].level_cond(0, lo, None, cnt),
        "cs1": lambda i: plans[i % n].level_cond(0, lo, hi, cnt, csum[1], 1),
        "cs2": lambda i: plans[i % n].level_cond(0, lo, hi, cnt, csum[2], 1),
        "cs3": lambda i: plans[i % n].level_cond(0, lo, hi, cnt, csum[3], 1),
        "cs8": lambda i: plans[i % n].level_cond(0, lo, hi, cnt, csum[8], 1),
        "cs3_lo": lambda i: plans[i % n].level_cond(0, lo, None, cnt, csum[3], 1),
        "cs3_in": lambda i: plans[i % n].level_cond(0, lo, hi, cnt, csum[3], 0),
        "cs3_neg": lambda i: plans[i % n].level_cond(8, lo, hi, cnt, csum[3], 0),
        "cs3x1": cs3x1,
        "cs3_block": lambda i: plans[i % n].level_cond(0, lob, hib, cntb, csumb, 1, (ncrms - nb) // 2, nb),
    }
    for T in (0,) + TS:
        runs[f"export{T}"] = lambda i, T=T: plans[i % n].export_device(f=fx[:T + 1] if T else fx[0])
        runs[f"stats{T}"] = stats(T)
    # the algorithmic bytes: the interior of the tracers the call needs, read once
    ntr = {"cnt": 1, "cnt_lo": 1, "cs1": 2, "cs2": 3, "cs3": 4, "cs8": 9, "cs3_lo": 4, "cs3_in": 3, "cs3_neg": 4, "cs3x1": 4}
    base = {"cnt": 0, "cnt_lo": 0, "cs1": 1, "cs2": 2, "cs3": 3, "cs8": 8, "cs3_lo": 3, "cs3x1": 3, "cs3_neg": 3}
    if a.only:
        res[a.only + "_ms"], res[a.only + "_ms_max"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_ms_max"] = timed(fn, steps)
        for k in ("cnt", "cs3", "stats3"):
            res[k + "_ms_again"], _ = timed(runs[k], steps)
        for k, t in ntr.items():
            res[k + "_gbs"] = t * one / res[k + "_ms"] / 1e6
        for k, T in base.items():
            res[f"ratio_{k}_over_export"] = res[k + "_ms"] / res[f"export{T}_ms"]
            res[f"ratio_{k}_over_stats"] = res[k + "_ms"] / res[f"stats{T}_ms"]
        ms = lambda k: f"{res[k + '_ms']:.4f}"
        print(f"{tag:12s} [{a.label}]: share in {frac:.2f}  cnt {ms('cnt')} ms ({res['cnt_gbs']:.0f} GB/s; lo alone {ms('cnt_lo')})  "
              + "  ".join(f"cs{T} {ms(f'cs{T}')} ({res[f'cs{T}_gbs']:.0f} GB/s; / (a) export {ms(f'export{T}')}: "
                          f"{res[f'ratio_cs{T}_over_export']:.3f}, / (b) stats {ms(f'stats{T}')}: {res[f'ratio_cs{T}_over_stats']:.3f})"
                          for T in TS)
              + f"  |  cs3 max {res['cs3_ms_max']:.4f} again {res['cs3_ms_again']:.4f}  lo alone {ms('cs3_lo')}  tc inside {ms('cs3_in')}  "
              f"tc above {ms('cs3_neg')}  three calls of one tracer {ms('cs3x1')}  block of {nb} {ms('cs3_block')}  |  cnt / (a) "
              f"{res['ratio_cnt_over_export']:.3f}  / (b) {res['ratio_cnt_over_stats']:.3f}", flush=True)
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
