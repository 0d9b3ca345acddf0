#!/usr/bin/env python3
"""Time of the per-level histograms of a resident plan's tracers (include/mpdata_hip.h 3ab), cold, at ncrms=65536 nx=32
nz=28 and at ncrms=4096 nx=32 nz=300 (a windowed plan), plans of four tracers (the binned tracer and three value tracers),
fp64 and fp32: consecutive calls go to different plans (field sets), as bench.py runs its steps, so no call finds its f in
the Infinity Cache.  Per call (torch events around a round of calls on the plans' stream, behind a wake-up: rounds until
two consecutive ones agree within 3 %); the MEDIAN of five rounds, with their minimum, maximum and spread = (max - min) /
median.  With tc = 0, the value tracers 1 .. T and nb equal-width bins over the field's range:
  cnt_nbN                 : cnt alone, N = 2, 4, 8, 16, 32 bins
  cs1_nbN, cs3_nbN        : cnt and bsum of T = 1, 3 value tracers, N = 8, 32
  cs3_nb8_block           : cs3_nb8 on a block of 64 instances
and the yardsticks in the same process on the same plans, calls that exist without 3ab (--no-yardsticks leaves them out):
  condxN, cond1xN, cond3xN : (a) N Plan.level_cond calls with lo = e_j, hi = e_{j+1} -- the route "bin by bin" this call
                            replaces --, cnt alone / with one / with three value tracers
  cond, cond1, cond3      : (b) ONE such call: the floor of one read of the same bytes
  export0, export1, export3 : (c) Plan.export_device of the T + 1 tracers
and from them the ratios and TB/s against the algorithmic bytes: (T + 1) nx nzm ncrms reals (the interior of the T + 1
tracers read once).  A ratio of two measurements whose distance is inside the larger of their spreads, or inside the 3 % by
which two processes differ, is marked unresolved.  Candidate kernels are libraries built outside the tree from variants of
mpdata_level_hist.hip (lane-private bins in LDS; other bin groups): run once per library (MPDATA_HIP_LIB names it), --tag
names the run and --json merges it into the file.  The result of one call per nb
is checked against torch on an exported copy (the counts exactly, the sums to rounding).  Needs no oracle and no reference
tree.
usage: python tools/level_hist_bench.py [--steps K] [--sets N] [--json PATH] [--tag NAME] [--no-f32] [--no-tall] [--no-yardsticks]"""
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
ap.add_argument("--no-yardsticks", action="store_true", help="the new call alone (candidate libraries)")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. cnt_nb32")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "library": os.path.basename(M.lib_path()), "device": torch.cuda.get_device_name(0)}
TP = 4                                                  # tracers of a plan
NBS_CNT, NBS_SUM, TS = (2, 4, 8, 16, 32), (8, 32), (1, 3)


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
    edges = {nb: [i / nb for i in range(nb + 1)] for nb in NBS_CNT}      # the synthetic f lies in [0, 1)
    cnt = {nb: torch.empty((nb, nzm, ncrms), dtype=tdt, device=dev) for nb in NBS_CNT}
    bsum = {(T, nb): torch.empty((T, nb, nzm, ncrms), dtype=tdt, device=dev) for T in TS for nb in NBS_SUM}
    cntb, bsumb = torch.empty((8, nzm, nblk), dtype=tdt, device=dev), torch.empty((3, 8, nzm, nblk), dtype=tdt, device=dev)
    lo, hi = (torch.empty((nzm, ncrms), dtype=tdt, device=dev) for _ in range(2))
    c1, s1 = torch.empty((nzm, ncrms), dtype=tdt, device=dev), {T: torch.empty((T, nzm, ncrms), dtype=tdt, device=dev) for T in TS}
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

    # the check first: cnt and bsum of three value tracers against torch on an exported copy
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    plans[0].export_device(f=fx)
    c = fx[0, :, 3:nx + 3, :]                           # (nzm, nx, ncrms)
    for nb in NBS_SUM:
        plans[0].level_hist(0, edges[nb], cnt[nb], bsum[(3, nb)], 1)
        torch.cuda.synchronize()
        e = torch.tensor(edges[nb], dtype=tdt, device=dev)
        for j in (0, nb // 2, nb - 1):
            inn = (c > e[j]) & (c <= e[j + 1])
            assert torch.equal(cnt[nb][j].double(), inn.sum(dim=1).double()), (tag, nb, j)
            want = torch.where(inn, fx[2, :, 3:nx + 3, :].double(), torch.zeros((), dtype=torch.float64, device=dev)).sum(dim=1)
            err = float((bsum[(3, nb)][1, j].double() - want).abs().max())
            assert err < 4 * nx * nx * eps, (tag, nb, j, err)
        del inn, want
    res["share_in_a_bin"] = float(cnt[32].sum() / (float(nx) * nzm * ncrms))
    del c
    torch.cuda.empty_cache()

    # (a): the bounds of every bin made once, outside the timed rounds
    bound = {} if a.no_yardsticks else {nb: [torch.full((nzm, ncrms), e, dtype=tdt, device=dev) for e in edges[nb]] for nb in NBS_CNT}

    def cond_x(nb, T):
        def f(i):
            for j in range(nb):
                plans[i % n].level_cond(0, bound[nb][j], bound[nb][j + 1], c1, s1[T] if T else None, 1)
        return f

    runs = {}
    for nb in NBS_CNT:
        runs[f"cnt_nb{nb}"] = lambda i, nb=nb: plans[i % n].level_hist(0, edges[nb], cnt[nb])
    for T in TS:
        for nb in NBS_SUM:
            runs[f"cs{T}_nb{nb}"] = lambda i, T=T, nb=nb: plans[i % n].level_hist(0, edges[nb], cnt[nb], bsum[(T, nb)], 1)
    runs["cs3_nb8_block"] = lambda i: plans[i % n].level_hist(0, edges[8], cntb, bsumb, 1, None, (ncrms - nblk) // 2, nblk)
    ntr = {k: 1 + (int(k[2]) if k.startswith("cs") else 0) for k in runs if not k.endswith("block")}
    if not a.no_yardsticks:
        lo.fill_(0.25); hi.fill_(0.5)
        for nb in NBS_CNT:
            runs[f"condx{nb}"] = cond_x(nb, 0)
        for T in TS:
            for nb in NBS_SUM:
                runs[f"cond{T}x{nb}"] = cond_x(nb, T)
        runs["cond"] = lambda i: plans[i % n].level_cond(0, lo, hi, c1)
        for T in TS:
            runs[f"cond{T}"] = lambda i, T=T: plans[i % n].level_cond(0, lo, hi, c1, s1[T], 1)
        for T in (0,) + TS:
            runs[f"export{T}"] = lambda i, T=T: plans[i % n].export_device(f=fx[:T + 1] if T else fx[0])
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
    for nb in NBS_CNT:
        ratio(f"cnt_nb{nb}", f"condx{nb}"); ratio(f"cnt_nb{nb}", "cond"); ratio(f"cnt_nb{nb}", "export0")
    for T in TS:
        for nb in NBS_SUM:
            ratio(f"cs{T}_nb{nb}", f"cond{T}x{nb}"); ratio(f"cs{T}_nb{nb}", f"cond{T}"); ratio(f"cs{T}_nb{nb}", f"export{T}")
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
