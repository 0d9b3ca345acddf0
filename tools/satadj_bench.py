#!/usr/bin/env python3
"""Time of the saturation adjustment of a resident plan's tracers (include/mpdata_hip.h 3y), cold, at ncrms=65536 nx=32
nz=28, with 25 tracers, and at ncrms=4096 nx=32 nz=300 (a windowed plan), fp64 and fp32: consecutive calls go to different
plans (field sets), as bench.py runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch events around
a loop of calls on the plans' stream, after a wake-up: batches of calls until the batch time has stopped falling, i.e. two
consecutive batches agree within 3 %; then the minimum AND the maximum of three batches, the run-to-run spread).

Plans of four tracers (th, tq, tn, tt) = (0, 1, 2, 3).  Three fields of th and tq, on rows whose pressure depends on the
level alone (1010 .. 150), by the recipe of tests/satadj_model.py (T1 tied to p, q = U(0, 1.6) qs(T1)), made on the device:
  dry     : q = U(0, 0.9) qs(T1): no cell saturated, no Newton step
  mix     : the recipe: about a third of the cells saturated, scattered, so nearly every wave iterates as long as its
            slowest cell
  sorted  : the cells of mix permuted within each level so that the most supersaturated go to the first instances: the
            saturated cells fill whole rows and whole waves, the dry ones the others -- no divergence between dry and
            saturated cells inside a wave
Each with ICE on and off and tt given and absent, gz, ncld and iters given:
  satadj_<field>_<ice|liq>_<tt|nott>
and  satadj_block (mix, ICE, tt, a block of 64 instances), and in the same process the yardsticks
  round_trip  : (a) Plan.export_device of th, tq + Plan.import_device of tn, tt -- the route a caller had before the call
                existed, without the caller's own kernel
  convert_all : (b) Plan.convert 2 -> 3 with q0, y, LIMIT and dsum -- the same two reads and two writes per cell with
                almost no arithmetic: the ratio says whether the call is bound by bytes or by the vector unit
and from them the ratios (a), (b) and (c) = mix / sorted, the price of divergence.  (d), the columns interleaved per lane,
is this tool run on libraries built with other MPDATA_SATADJ_NC (MPDATA_HIP_LIB names the library; --tag names the run).
The result of one call is checked against a torch statement of the definition on the exported copies (to rounding: torch
may contract and iterate in another order of operations).  Needs no oracle and no reference tree.  Prints one line per
measurement and, with --json PATH, writes them all there.
usage: python tools/satadj_bench.py [--steps K] [--sets N] [--json PATH] [--no-f32] [--no-tall] [--no-wide] [--quick]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch

import codesign_kernels_amd as M
from satadj_model import PAR

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--block", type=int, default=64, help="instances of the block case")
ap.add_argument("--json", default=None)
ap.add_argument("--tag", default=None, help="a name for the run in the JSON (the library's MPDATA_SATADJ_NC)")
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--no-wide", action="store_true", help="no 25-tracer plan")
ap.add_argument("--quick", action="store_true", help="the mix field with ICE and tt and without both, and convert_all, alone")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0), "tag": a.tag, "lib": os.path.basename(M.lib_path())}
par = M.SatadjParams(**PAR)


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


def curve(c, dc, T, p):
    x = (T - PAR["t0"]).clamp_min(PAR["xmin"])
    es, de = torch.full_like(x, c[8]), torch.full_like(x, dc[8])
    for j in range(7, -1, -1):
        es, de = c[j] + x * es, dc[j] + x * de
    return PAR["eps"] * es / torch.maximum(p - es, es), PAR["eps"] * de / p


def sat(T, p, ice):
    """(qs, dq, L, dL) of the definition in torch, float64"""
    qw, dw = curve(PAR["esw"], PAR["desw"], T, p)
    lv, ls = PAR["lv"], PAR["ls"]
    if not ice:
        return qw, dw, torch.full_like(T, lv), torch.zeros_like(T)
    qi, di = curve(PAR["esi"], PAR["desi"], T, p)
    an = 1.0 / (PAR["tmax"] - PAR["tmin"])
    om = ((T - PAR["tmin"]) * an).clamp(0.0, 1.0)
    mixed = (om > 0) & (om < 1)
    return om * qw + (1 - om) * qi, om * dw + (1 - om) * di, lv + (1 - om) * (ls - lv), torch.where(mixed, an * (ls - lv), 0.0)


def newton(h, q, p, gz, ice):
    """(qn, T) of the definition in torch, float64, every cell iterated to the definition's stop"""
    qq = q.clamp_min(0)
    T1 = h - gz
    qs, _, _, _ = sat(T1, p, ice)
    wet = qq > qs
    T, act = T1.clone(), wet.clone()
    d, dq = torch.zeros_like(T), torch.zeros_like(T)
    for _ in range(PAR["maxit"]):
        nqs, ndq, L, dL = sat(T, p, ice)
        e = qq - nqs
        nd = -((T1 - T) + L * e) / ((dL * e - L * ndq) - 1)
        qs, dq, d = torch.where(act, nqs, qs), torch.where(act, ndq, dq), torch.where(act, nd, d)
        T = torch.where(act, T + nd, T)
        act = act & (nd.abs() > PAR["tol"])
        if not bool(act.any()):
            break
    return torch.where(wet, (qq - (qs + dq * d)).clamp_min(0), 0.0), T, wet


def measure(tag, shape, tdt, eb, sets, steps, tall, T):
    ncrms, nx, nz = shape
    nzm = nz - 1
    th, tq, tn, tt = 0, 1, T - 2, T - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, 2)
    ssh = M.satadj_shapes(ncrms, nx, nz)
    nb = min(a.block, ncrms)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo)
    plev = torch.linspace(1010.0, 150.0, nzm, device=dev, dtype=torch.float64)
    pres = plev[:, None].expand(nzm, ncrms).contiguous().to(tdt)
    gz = (torch.linspace(0.0, 120.0, nzm, device=dev, dtype=torch.float64)[:, None].expand(nzm, ncrms)).contiguous().to(tdt)
    ncld, iters = torch.empty(ssh["ncld"], dtype=tdt, device=dev), torch.empty(ssh["iters"], dtype=tdt, device=dev)
    p3, g3 = pres.double()[:, None, :], gz.double()[:, None, :]

    def field(kind, seed):
        """(2, nzm, nx+6, ncrms): th and tq"""
        gg = torch.Generator(device=dev).manual_seed(seed)
        u = lambda lo, hi: torch.rand((nzm, nx + 6, ncrms), generator=gg, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo)
        T1 = 225.0 + 80.0 * (p3 - 150.0) / 860.0 + u(-6.0, 6.0)
        h = (T1 + g3).to(tdt)
        qs = sat(h.double() - g3, p3, True)[0]
        q = u(0.0, 0.9 if kind == "dry" else 1.6) * qs
        if kind == "sorted":
            # within each level the cells of the interior, most supersaturated first, dealt out instance by instance
            ratio = (q / qs)[:, 3:nx + 3, :].permute(0, 2, 1).reshape(nzm, -1)
            order = ratio.argsort(dim=1, descending=True)
            for src in (h, q):
                v = src[:, 3:nx + 3, :].permute(0, 2, 1).reshape(nzm, -1)
                src[:, 3:nx + 3, :] = torch.gather(v, 1, order).reshape(nzm, ncrms, nx).permute(0, 2, 1)
        return torch.stack([h, q.to(tdt)])

    plans = []
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        z = torch.zeros(M.shapes(ncrms, nx, nz, 1)["f"], dtype=tdt, device=dev)
        for t in range(T):
            p.import_device(f=z, first_tracer=t)
        plans.append(p)
    del z
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    cells = float(nx) * nzm * ncrms
    alg = cells * eb * 4                                   # two tracers read, two written (tt given)
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows), "algorithmic_bytes_tt": alg,
           "algorithmic_bytes_nott": cells * eb * 3, "round_trip_bytes": float(nx + 6) * nzm * ncrms * eb * 8}

    def load(kind):
        for s, p in enumerate(plans):
            p.import_device(f=field(kind, 100 + s), first_tracer=th)
        torch.cuda.synchronize()

    # the check first: one call with everything on the mix against torch on the exported copies
    load("mix")
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    plans[0].export_device(f=fx, first_tracer=th)
    torch.cuda.synchronize()
    f0 = fx.clone().double()
    plans[0].satadj(th, tq, tn, pres, par, tt, gz, M.SATADJ_ICE, ncld, iters)
    plans[0].export_device(f=fx, first_tracer=tn)
    torch.cuda.synchronize()
    qn, Tn, wet = newton(f0[0, :, 3:nx + 3], f0[1, :, 3:nx + 3], p3, g3, True)
    share = float(wet.double().mean())
    # (a Newton step multiplies a rounding error of T by L dq ~ up to 10; the stop at |d| <= tol leaves both sides within
    # tol * |d| of the root, far below this bound)
    assert float((fx[1, :, 3:nx + 3].double() - Tn).abs().max()) < 1e-3 * (1 if eb == 8 else 50), tag
    assert float((fx[0, :, 3:nx + 3].double() - qn).abs().max()) < 1e-6 * (1 if eb == 8 else 50), tag
    assert abs(float(ncld.double().sum()) - float((qn > 0).double().sum())) <= 1e-4 * cells, tag
    assert 0.15 <= share <= 0.6 and 1 <= float(iters.max()) <= 7, (tag, share, float(iters.max()))
    res["saturated_share_mix"] = share
    res["iters_max_mix"] = float(iters.max())
    del f0, qn, Tn, wet
    torch.cuda.empty_cache()

    def round_trip(i):
        plans[i % n].export_device(f=fx, first_tracer=th)
        plans[i % n].import_device(f=fx, first_tracer=tn)

    csh = M.convert_shapes(ncrms, nx, nz)
    r, q0, y = rnd(csh["r"], 0.005, 0.02).to(tdt), rnd(csh["q0"], 0.3, 0.6).to(tdt), rnd(csh["y"], 0.5, 1.5).to(tdt)
    dsum = torch.empty(csh["dsum"], dtype=tdt, device=dev)
    presb, gzb = pres[:, :nb].contiguous(), gz[:, :nb].contiguous()

    def sat_call(ice, tt_on):
        return lambda i: plans[i % n].satadj(th, tq, tn, pres, par, tt if tt_on else -1, gz, M.SATADJ_ICE if ice else 0, ncld, iters)

    variants = [("ice_tt", True, True), ("liq_nott", False, False)] if a.quick else \
        [("ice_tt", True, True), ("ice_nott", True, False), ("liq_tt", False, True), ("liq_nott", False, False)]
    for kind in (("mix",) if a.quick else ("mix", "dry", "sorted")):
        if kind != "mix":
            load(kind)
        for vn, ice, tt_on in variants:
            k = f"satadj_{kind}_{vn}"
            res[k + "_ms"], res[k + "_ms_max"] = timed(sat_call(ice, tt_on), steps)
        if kind == "mix":
            res["satadj_mix_ice_tt_ms_again"], _ = timed(sat_call(True, True), steps)
            if not a.quick:
                res["satadj_block_ms"], res["satadj_block_ms_max"] = timed(
                    lambda i: plans[i % n].satadj(th, tq, tn, presb, par, tt, gzb, M.SATADJ_ICE, sl0=(ncrms - nb) // 2, n=nb), steps)
    res["convert_all_ms"], res["convert_all_ms_max"] = timed(lambda i: plans[i % n].convert(tn, tt, r, q0, y, M.CONVERT_LIMIT, dsum), steps)
    if not a.quick:
        res["round_trip_ms"], res["round_trip_ms_max"] = timed(round_trip, steps)
        res["convert_all_ms_again"], _ = timed(lambda i: plans[i % n].convert(tn, tt, r, q0, y, M.CONVERT_LIMIT, dsum), steps)
        for kind in ("mix", "dry", "sorted"):
            res[f"ratio_a_{kind}_ice_tt_over_round_trip"] = res[f"satadj_{kind}_ice_tt_ms"] / res["round_trip_ms"]
            for vn, _, _ in variants:
                res[f"ratio_b_{kind}_{vn}_over_convert"] = res[f"satadj_{kind}_{vn}_ms"] / res["convert_all_ms"]
        for vn, _, _ in variants:
            res[f"ratio_c_mix_over_sorted_{vn}"] = res[f"satadj_mix_{vn}_ms"] / res[f"satadj_sorted_{vn}_ms"]
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
    res["convert_all_gbs"] = alg / res["convert_all_ms"] / 1e6
    for k in [k for k in res if k.startswith("satadj_") and k.endswith("_ms") and "block" not in k]:
        res[k[:-3] + "_gbs"] = res["algorithmic_bytes_" + ("nott" if k.endswith("nott_ms") else "tt")] / res[k] / 1e6
    print(f"{tag:12s}: " + "  ".join(f"{k[:-3]} {v:.4f}" for k, v in res.items() if k.endswith("_ms")), flush=True)
    if not a.quick:
        print(f"{tag:12s}: " + "  ".join(f"{k} {v:.3f}" for k, v in res.items() if k.startswith("ratio_")), flush=True)
    for p in plans:
        p.close()
    del plans, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
prec = [("f64", torch.float64, 8)] + ([] if a.no_f32 else [("f32", torch.float32, 4)])
cases = [(t, tuple(a.shape), tdt, eb, a.sets, False, 4) for t, tdt, eb in prec]
if not a.no_wide and not a.quick:
    cases += [(t + "_25tr", tuple(a.shape), tdt, eb, 2, False, 25) for t, tdt, eb in prec]
if not a.no_tall and not a.quick:
    cases += [(t + "_tall", tuple(a.tall_shape), tdt, eb, a.sets, True, 4) for t, tdt, eb in prec]
for tag, shape, tdt, eb, sets, tall, T in cases:
    measure(tag, shape, tdt, eb, sets, a.steps, tall, T)
M.set_tall_columns(0)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
