#!/usr/bin/env python3
"""Time of the per-level covariance of two tracers of a resident plan (include/mpdata_hip.h 3u), cold, at ncrms=65536 nx=32
nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), two tracers, fp64 and fp32: consecutive calls go to different
plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch events
around a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped falling,
i.e. two consecutive batches agree within 3 %; then the minimum AND the maximum of three batches, the run-to-run spread):
  raw_ab, raw_aa          : Plan.level_cov, mode LEVEL_COV_RAW, tracers (0, 1) and (0, 0)          -- the one-pass form
  given_ab, given_aa      : both profiles given                                                    -- the one-pass form
  central_ab, central_aa  : both means formed (nx <= 32: the kept form; else the re-read form)
  central_ab_out          : central_ab with mean_a and mean_b written
  central_ba              : tracers (1, 0): the negative offset between the two streams
  central_block           : central_ab on a block of 64 instances
and two yardsticks in the same process, calls that exist without 3u:
  export2  : (a) Plan.export_device of both tracers of f -- the route a caller had before the call existed, without the
             caller's own kernel: the comparison that decides whether the call pays
  stats2   : (b) two Plan.level_stats calls (sum), one tracer each -- the same bytes read once, without the products
and from them the ratios and GB/s against the algorithmic bytes: 2 nx nzm ncrms reals (the interior of two tracers read
once; one tracer for ta == tb).  The kept form against the re-read form: run the tool once more on a library whose
mpdata_level_cov.hip was compiled with -DMPDATA_LEVEL_COV_KEPT_NX1=0 -DMPDATA_LEVEL_COV_KEPT_NX2=0 (MPDATA_HIP_LIB names
it); --label tags the output.  The result of one call is checked against torch on an exported copy (to rounding: torch sums
in another order).  Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes
them all there.
usage: python tools/level_cov_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--label TEXT]"""
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
ap.add_argument("--label", default="default", help="which build of the library this is (kept / re-read)")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. central_ab")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "label": a.label, "library": os.path.basename(M.lib_path()),
       "device": torch.cuda.get_device_name(0)}
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
    csh = M.level_cov_shapes(ncrms, nx, nz)
    nb = min(a.block, ncrms)
    bsh = M.level_cov_shapes(nb, nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    ma, mb = rnd(csh["ma"], 0.3, 0.6), rnd(csh["mb"], 0.3, 0.6)
    cov, mean_a, mean_b = (torch.empty(csh[k], dtype=tdt, device=dev) for k in ("cov", "mean_a", "mean_b"))
    covb = torch.empty(bsh["cov"], dtype=tdt, device=dev)
    ssum = torch.empty(csh["cov"], dtype=tdt, device=dev)
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
    one = float(nx) * nzm * ncrms * eb                   # the interior of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows), "ab_bytes": 2 * one, "aa_bytes": one,
           "stats2_bytes": 2 * one, "export2_bytes": 4 * one * (nx + 6) / nx}

    # the check first: the central call with the mean outputs, the one about given profiles and the RAW one against torch on
    # an exported copy
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    plans[0].export_device(f=fx)
    torch.cuda.synchronize()
    fa, fb = fx[0, :, 3:nx + 3, :].double(), fx[1, :, 3:nx + 3, :].double()      # (nzm, nx, ncrms)
    scale = float(fa.abs().max() * fb.abs().max()) * nx + 1.0
    plans[0].level_cov(0, 1, cov, mean_a=mean_a, mean_b=mean_b)
    torch.cuda.synchronize()
    wa, wb = fa.mean(dim=1), fb.mean(dim=1)
    assert float((mean_a.double() - wa).abs().max()) < 2 * nx * eps and float((mean_b.double() - wb).abs().max()) < 2 * nx * eps, tag
    want = ((fa - wa.unsqueeze(1)) * (fb - wb.unsqueeze(1))).sum(dim=1)
    err = float((cov.double() - want).abs().max() / scale)
    assert err < 8 * nx * eps, (tag, "central", err)
    plans[0].level_cov(1, 0, cov, ma, mb)
    torch.cuda.synchronize()
    want = ((fb - ma.double().unsqueeze(1)) * (fa - mb.double().unsqueeze(1))).sum(dim=1)
    err = float((cov.double() - want).abs().max() / scale)
    assert err < 8 * nx * eps, (tag, "given", err)
    plans[0].level_cov(0, 0, cov, mode=M.LEVEL_COV_RAW)
    torch.cuda.synchronize()
    err = float((cov.double() - (fa * fa).sum(dim=1)).abs().max() / scale)
    assert err < 8 * nx * eps and float(cov.min()) >= 0, (tag, "raw", err)
    del fa, fb, wa, wb, want
    torch.cuda.empty_cache()

    def stats2(i):
        plans[i % n].level_stats(sum=ssum, first_tracer=0)
        plans[i % n].level_stats(sum=ssum, first_tracer=1)

    RAW = M.LEVEL_COV_RAW
    runs = {
        "raw_ab": lambda i: plans[i % n].level_cov(0, 1, cov, mode=RAW),
        "raw_aa": lambda i: plans[i % n].level_cov(0, 0, cov, mode=RAW),
        "given_ab": lambda i: plans[i % n].level_cov(0, 1, cov, ma, mb),
        "given_aa": lambda i: plans[i % n].level_cov(0, 0, cov, ma, mb),
        "central_ab": lambda i: plans[i % n].level_cov(0, 1, cov),
        "central_aa": lambda i: plans[i % n].level_cov(0, 0, cov),
        "central_ab_out": lambda i: plans[i % n].level_cov(0, 1, cov, mean_a=mean_a, mean_b=mean_b),
        "central_ba": lambda i: plans[i % n].level_cov(1, 0, cov),
        "central_block": lambda i: plans[i % n].level_cov(0, 1, covb, sl0=(ncrms - nb) // 2, n=nb),
        "export2": lambda i: plans[i % n].export_device(f=fx),
        "stats2": stats2,
    }
    if a.only:
        res[a.only + "_ms"], res[a.only + "_ms_max"] = timed(runs[a.only], steps)
        print(f"{tag:12s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_ms_max"] = timed(fn, steps)
        for k in ("central_ab", "central_aa", "stats2"):
            res[k + "_ms_again"], _ = timed(runs[k], steps)
        for c in ("raw_ab", "given_ab", "central_ab", "central_ab_out", "central_ba"):
            res[c + "_gbs"] = res["ab_bytes"] / res[c + "_ms"] / 1e6
            for k in ("export2", "stats2"):
                res[f"ratio_{c}_over_{k}"] = res[c + "_ms"] / res[k + "_ms"]
        for c in ("raw_aa", "given_aa", "central_aa"):
            res[c + "_gbs"] = res["aa_bytes"] / res[c + "_ms"] / 1e6
        for k in ("export2", "stats2"):
            res[k + "_gbs"] = res[k + "_bytes"] / res[k + "_ms"] / 1e6
        ms = lambda k: f"{res[k + '_ms']:.4f}"
        print(f"{tag:12s} [{a.label}]: ta != tb: RAW {ms('raw_ab')} ms ({res['raw_ab_gbs']:.0f} GB/s)  given {ms('given_ab')} "
              f"({res['given_ab_gbs']:.0f})  central {ms('central_ab')} (max {res['central_ab_ms_max']:.4f}, again "
              f"{res['central_ab_ms_again']:.4f}; {res['central_ab_gbs']:.0f} GB/s)  with means out {ms('central_ab_out')}  (1, 0) "
              f"{ms('central_ba')}  block of {nb} {ms('central_block')}  |  ta == tb: RAW {ms('raw_aa')} ({res['raw_aa_gbs']:.0f} "
              f"GB/s)  given {ms('given_aa')}  central {ms('central_aa')} (again {res['central_aa_ms_again']:.4f}; "
              f"{res['central_aa_gbs']:.0f} GB/s)  |  (a) export of both tracers {ms('export2')} ({res['export2_gbs']:.0f} GB/s)  (b) "
              f"two level_stats {ms('stats2')} (again {res['stats2_ms_again']:.4f}; {res['stats2_gbs']:.0f} GB/s)  |  central / (a) "
              f"{res['ratio_central_ab_over_export2']:.3f}  / (b) {res['ratio_central_ab_over_stats2']:.3f}  RAW / (a) "
              f"{res['ratio_raw_ab_over_export2']:.3f}  / (b) {res['ratio_raw_ab_over_stats2']:.3f}", flush=True)
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
