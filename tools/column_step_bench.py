#!/usr/bin/env python3
"""Time of the fused column step of a resident plan (include/mpdata_hip.h 3q), one tracer, cold, at ncrms=65536 nx=32
nz=28, fp64 and fp32: consecutive calls go to different plans (field sets) with their own s and wp, as bench.py runs its
steps, so no call finds its f, its s or its wp in the Infinity Cache.  Per call (torch events around a loop of calls on
the plans' stream, after a wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive
batches agree within 3 %):
  all4                : Plan.column_step_device with all four stages (source, subside, sediment, vsolve), no psfc
  all4_psfc           : the same with psfc
  only_source .. only_vsolve : the four single-stage forms of the new call
and, in the same process, calls that exist without 3q (their code is unchanged):
  cell_add, subside, sediment, vsolve : the four single calls, no horizontal sums, no psfc
  round_trip          : Plan.export_device + Plan.import_device of f alone
and from them: the ratio of all4 to the SUM of the four single calls, the rate of all4 on its algorithmic bytes (f read and
written once, s and wp read once: 4 nx nzm ncrms reals), and each single-stage form against its sibling.  Before the
timing one all4 call is checked bit for bit against the sequence of the four single calls on a second plan with the same
field (interior columns).  Needs no oracle and no reference tree.  Prints one line per measurement and, with --json PATH,
writes them all there.
usage: python tools/column_step_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32]"""
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
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. all4")
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


def measure(tag, shape, tdt, eb, sets, steps):
    ncrms, nx, nz = shape
    nzm = nz - 1
    sh = M.shapes(ncrms, nx, nz, 1)
    csh = M.column_step_shapes(ncrms, nx, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    psfc = torch.empty(csh["psfc"], dtype=tdt, device=dev)
    # (small values of both signs and a diagonally dominant matrix: hundreds of timed calls on one field stay finite)
    cb, cc = rnd(csh["cb"], -0.002, 0.002), rnd(csh["cc"], -0.002, 0.002)
    lo, up = rnd(csh["lo"], -0.4, 0.0), rnd(csh["up"], -0.4, 0.0)
    di = (1.0 - lo.double() - up.double()).to(tdt)
    plans, ss, wps = [], [], []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets + 1):     # (the last plan is the check's second plan)
        p = M.Plan(ncrms, nx, nz, 1, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and p.level_windows == 1
        p.set_stream()
        p.set_timing(False)
        seed = 0 if s == sets else s                     # (the check's plan holds the fields of plan 0)
        M.fill_synthetic(ftmp, "f", 100 + seed, 1)
        p.import_device(f=ftmp)
        g2 = torch.Generator(device=dev).manual_seed(500 + seed)
        for k in ("rho", "adz"):
            p.import_device(**{k: torch.rand(sh[k], generator=g2, device=dev, dtype=torch.float64).mul_(0.5).add_(0.5).to(tdt)})
        plans.append(p)
        ss.append(rnd(csh["s"], -0.004, 0.004))
        wps.append(rnd(csh["wp"], -0.002, 0.008))
    check = plans.pop()
    ss.pop(); wps.pop()
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    fy = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb                        # bytes of one column of all instances
    alg = col * 4 * nx                                   # the interior of f read and written, s and wp read
    res = {"shape": [ncrms, nx, nz], "algorithmic_bytes": alg, "round_trip_bytes": col * 4 * (nx + 6)}

    # the check first: plan 0 takes the fused call, the check plan (the same f, rho, adz) the four single calls
    plans[0].column_step_device(s=ss[0], c=-150.0, mode=M.CELL_ADD_CLIP, cb=cb, cc=cc, wp=wps[0], psfc=psfc, lo=lo, di=di, up=up)
    check.cell_add(ss[0], -150.0, M.CELL_ADD_CLIP)
    check.subside(cb, cc)
    check.sediment(wps[0])
    check.vsolve(lo, di, up)
    plans[0].export_device(f=fx)
    check.export_device(f=fy)
    torch.cuda.synchronize()
    assert torch.equal(fx[:, 3:nx + 3].view(torch.uint8), fy[:, 3:nx + 3].view(torch.uint8)), f"{tag}: the fused call is not the sequence"
    assert bool(torch.isfinite(fx).all()) and float((fx[:, 3:nx + 3] == 0).double().mean()) < 0.9
    check.close()
    del fy
    torch.cuda.empty_cache()

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    P = lambda i: plans[i % n]
    runs = {
        "all4": lambda i: P(i).column_step_device(s=ss[i % n], c=0.75, cb=cb, cc=cc, wp=wps[i % n], lo=lo, di=di, up=up),
        "all4_psfc": lambda i: P(i).column_step_device(s=ss[i % n], c=0.75, cb=cb, cc=cc, wp=wps[i % n], psfc=psfc, lo=lo, di=di, up=up),
        "only_source": lambda i: P(i).column_step_device(s=ss[i % n], c=0.75),
        "only_subside": lambda i: P(i).column_step_device(cb=cb, cc=cc),
        "only_sediment": lambda i: P(i).column_step_device(wp=wps[i % n]),
        "only_vsolve": lambda i: P(i).column_step_device(lo=lo, di=di, up=up),
        "cell_add": lambda i: P(i).cell_add(ss[i % n], 0.75),
        "subside": lambda i: P(i).subside(cb, cc),
        "sediment": lambda i: P(i).sediment(wps[i % n]),
        "vsolve": lambda i: P(i).vsolve(lo, di, up),
        "round_trip": round_trip,
    }
    if a.only:
        res[a.only + "_ms"] = timed(runs[a.only], steps)
        print(f"{tag:5s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"] = timed(fn, steps)
        res["all4_ms_again"] = timed(runs["all4"], steps)
        res["sum_of_single_calls_ms"] = sum(res[k + "_ms"] for k in ("cell_add", "subside", "sediment", "vsolve"))
        res["ratio_all4_over_sum"] = res["all4_ms"] / res["sum_of_single_calls_ms"]
        res["ratio_all4_over_round_trip"] = res["all4_ms"] / res["round_trip_ms"]
        res["all4_gbs"] = alg / res["all4_ms"] / 1e6
        for new, old in (("only_source", "cell_add"), ("only_subside", "subside"), ("only_sediment", "sediment"), ("only_vsolve", "vsolve")):
            res[f"ratio_{new}_over_{old}"] = res[new + "_ms"] / res[old + "_ms"]
        print(f"{tag:5s}: all four {res['all4_ms']:.4f} ms ({res['all4_gbs']:.0f} GB/s; again {res['all4_ms_again']:.4f}; with psfc "
              f"{res['all4_psfc_ms']:.4f})  sum of the four single calls {res['sum_of_single_calls_ms']:.4f}  ratio "
              f"{res['ratio_all4_over_sum']:.3f}  export + import of f {res['round_trip_ms']:.4f}", flush=True)
        for new, old in (("only_source", "cell_add"), ("only_subside", "subside"), ("only_sediment", "sediment"), ("only_vsolve", "vsolve")):
            print(f"{tag:5s}: {new} {res[new + '_ms']:.4f} ms  {old} {res[old + '_ms']:.4f} ms  ratio {res[f'ratio_{new}_over_{old}']:.3f}",
                  flush=True)
    for p in plans:
        p.close()
    del plans, ss, wps, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
cases = [("f64", tuple(a.shape), torch.float64, 8)]
if not a.no_f32:
    cases.append(("f32", tuple(a.shape), torch.float32, 4))
for tag, shape, tdt, eb in cases:
    measure(tag, shape, tdt, eb, a.sets, a.steps)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
