#!/usr/bin/env python3
"""Time of the per-level updraft / downdraft sampling of a resident plan (include/mpdata_hip.h 3ac), cold, at ncrms=65536
nx=32 nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), plans of nine tracers (the condition tracer and eight value
tracers) that hold u and w, fp64 and fp32: consecutive calls go to different plans (field sets), as bench.py runs its steps,
so no call finds its fields in the Infinity Cache.  Per call (torch events around a round of calls on the plans' stream,
behind a wake-up: rounds until two consecutive ones agree within 3 %); the MEDIAN of five rounds, with their minimum,
maximum and spread = (max - min) / median.  With tc = 0, lo = 0.25, hi = 0.75 on the synthetic f in [0, 1), the thresholds
wup = 0.25, wdn = -0.25 on the synthetic w in [-0.5, 0.5) and the value tracers 1 .. T:
  cw                      : cnt and wsum alone
  fsT, fwT                : fsum / fsum and wfsum of T = 1, 3, 8 value tracers
  fw3_block               : fw3 on a block of 64 instances
and the yardsticks in the same process on the same plans, calls that exist without 3ac (--no-yardsticks leaves them out):
  cond, condT             : Plan.level_cond with the same condition and value tracers (cnt alone / cnt and csum): one
                            stream fewer per walk -- no w
  courant                 : Plan.courant (clev): the same two w streams, and u
  exportT                 : Plan.export_device of the T + 1 tracers: the old route, which still leaves the caller's kernel
                            and their copy of w
and from them the ratios and TB/s against the algorithmic bytes: (2 + 1 + T) nx nzm ncrms reals (the interior of w twice
and of the T + 1 tracers once).  A ratio of two measurements whose distance is inside the larger of their spreads, or
inside the 3 % by which two processes differ, is marked unresolved.  One call is checked against torch on an exported copy
of f and the w that was imported (the counts exactly, the sums to rounding).  Needs no oracle and no reference tree.
usage: python tools/level_draft_bench.py [--steps K] [--sets N] [--json PATH] [--tag NAME] [--no-f32] [--no-tall] [--no-yardsticks]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--block", type=int, default=64, help="instances of the block case")
ap.add_argument("--json", default=None)
ap.add_argument("--tag", default="as_built", help="which build of the library this is")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--no-yardsticks", action="store_true", help="the new call alone")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. fw8")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "library": os.path.basename(M.lib_path()), "device": torch.cuda.get_device_name(0)}
TP = 9                                                  # tracers of a plan
TS = (1, 3, 8)
WUP, WDN = 0.25, -0.25


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps):
    """-> (median, min, max) of five rounds behind the wake-up"""
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the round time has stopped falling
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
    nblk = min(a.block, ncrms)
    sh = M.level_draft_shapes(ncrms, nx, nz, max(TS))
    cnt, wsum = (torch.empty(sh["cnt"], dtype=tdt, device=dev) for _ in range(2))
    fsum, wfsum = (torch.empty(sh["fsum"], dtype=tdt, device=dev) for _ in range(2))
    shb = M.level_draft_shapes(nblk, nx, nz, 3)
    fsb, wfb = (torch.empty(shb["fsum"], dtype=tdt, device=dev) for _ in range(2))
    lob, hib = (torch.full((nzm, nblk), v, dtype=tdt, device=dev) for v in (0.25, 0.75))
    lo, hi = (torch.empty((nzm, ncrms), dtype=tdt, device=dev) for _ in range(2))
    lo.fill_(0.25); hi.fill_(0.75)
    c1, s1 = torch.empty((nzm, ncrms), dtype=tdt, device=dev), torch.empty((max(TS), nzm, ncrms), dtype=tdt, device=dev)
    clev = torch.empty((nzm, ncrms), dtype=tdt, device=dev)
    shp = M.shapes(ncrms, nx, nz, 1)
    plans = []
    ftmp = torch.empty(shp["f"], dtype=tdt, device=dev)
    arrs = {k: torch.empty(shp[k], dtype=tdt, device=dev) for k in ("u", "w", "rho", "rhow", "adz")}
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, TP, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        for k, t in arrs.items():
            M.fill_synthetic(t, k, 100 + 10 * s, 1)
        p.import_device(**arrs)
        for t in range(TP):
            M.fill_synthetic(ftmp, "f", 100 + 10 * s + t, 1)
            p.import_device(f=ftmp, first_tracer=t)
        plans.append(p)
    torch.cuda.synchronize()
    del ftmp
    n = len(plans)
    one = float(nx) * nzm * ncrms * eb                   # the interior of one tracer
    res = {"shape": [ncrms, nx, nz], "tracers": TP, "level_windows": int(plans[0].level_windows), "tracer_bytes": one}

    # the check first, on the last plan (arrs holds its velocities): against torch on an exported copy of tracers 0 and 2
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    fx = torch.empty(M.shapes(ncrms, nx, nz, 3)["f"], dtype=tdt, device=dev)
    plans[-1].export_device(f=fx)
    plans[-1].level_draft(0, lo, hi, WUP, WDN, cnt, wsum, fsum[:3], wfsum[:3], 0)
    torch.cuda.synchronize()
    w = arrs["w"]                                        # (nz, nx + 4, ncrms)
    wk1 = torch.cat([w[1:nzm, 2:nx + 2], torch.zeros((1, nx, ncrms), dtype=tdt, device=dev)], dim=0)
    wc = 0.5 * (w[:nzm, 2:nx + 2] + wk1)
    c = fx[0, :, 3:nx + 3, :]
    inn = (c > 0.25) & (c <= 0.75)
    up, dn = wc > WUP, wc < WDN
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for k, m in enumerate((inn & up, inn & dn, inn & ~up & ~dn)):
        assert torch.equal(cnt[k].double(), m.sum(dim=1).double()), (tag, "cnt", k)
        for got, val in ((wsum[k], wc), (fsum[2, k], fx[2, :, 3:nx + 3, :]), (wfsum[2, k], wc * fx[2, :, 3:nx + 3, :])):
            err = float((got.double() - torch.where(m, val.double(), zero).sum(dim=1)).abs().max())
            assert err < 4 * nx * nx * eps, (tag, k, err)
    res["share_up_down_env"] = [float(cnt[k].sum() / (float(nx) * nzm * ncrms)) for k in range(3)]
    del fx, w, wk1, wc, c, inn, up, dn, m
    fx = None
    torch.cuda.empty_cache()

    runs = {"cw": lambda i: plans[i % n].level_draft(0, lo, hi, WUP, WDN, cnt, wsum)}
    for T in TS:
        runs[f"fs{T}"] = lambda i, T=T: plans[i % n].level_draft(0, lo, hi, WUP, WDN, None, None, fsum[:T], None, 1)
        runs[f"fw{T}"] = lambda i, T=T: plans[i % n].level_draft(0, lo, hi, WUP, WDN, None, None, fsum[:T], wfsum[:T], 1)
    runs["fw3_block"] = lambda i: plans[i % n].level_draft(0, lob, hib, WUP, WDN, None, None, fsb, wfb, 1, (ncrms - nblk) // 2, nblk)
    ntr = {"cw": 3}
    ntr.update({f"{k}{T}": 3 + T for T in TS for k in ("fs", "fw")})
    if not a.no_yardsticks:
        fx = torch.empty(M.shapes(ncrms, nx, nz, max(TS) + 1)["f"], dtype=tdt, device=dev)
        runs["cond"] = lambda i: plans[i % n].level_cond(0, lo, hi, c1)
        for T in TS:
            runs[f"cond{T}"] = lambda i, T=T: plans[i % n].level_cond(0, lo, hi, c1, s1[:T], 1)
            runs[f"export{T}"] = lambda i, T=T: plans[i % n].export_device(f=fx[:T + 1])
        runs["courant"] = lambda i: plans[i % n].courant(clev=clev)
    if a.only:
        runs = {a.only: runs[a.only]}
    for k, fn in runs.items():
        res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"] = timed(fn, steps)
        res[k + "_spread"] = (res[k + "_ms_max"] - res[k + "_ms_min"]) / res[k + "_ms"]
        print(f"{tag:10s} [{a.tag}] {k:14s} {res[k + '_ms']:.4f} ms  (min {res[k + '_ms_min']:.4f} max {res[k + '_ms_max']:.4f})", flush=True)
    for k, t in ntr.items():
        if k + "_ms" in res:
            res[k + "_tbs"] = t * one / res[k + "_ms"] / 1e9

    def ratio(k, y):
        if k + "_ms" in res and y + "_ms" in res:
            r = res[k + "_ms"] / res[y + "_ms"]
            res[f"ratio_{k}_over_{y}"] = r
            res[f"ratio_{k}_over_{y}_resolved"] = bool(abs(r - 1) > max(0.03, res[k + "_spread"], res[y + "_spread"]))
    ratio("cw", "cond"); ratio("cw", "courant")
    for T in TS:
        for k in (f"fs{T}", f"fw{T}"):
            ratio(k, f"cond{T}"); ratio(k, "courant"); ratio(k, f"export{T}")
        ratio(f"fw{T}", f"fs{T}")
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
print(json.dumps({a.tag: out}))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    allr = json.load(open(a.json)) if os.path.exists(a.json) else {}
    allr[a.tag] = out
    with open(a.json, "w") as fh:
        json.dump(allr, fh, indent=1)
