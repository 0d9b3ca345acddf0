#!/usr/bin/env python3
"""Time of the implicit vertical diffusion of a resident plan with a per-cell diffusivity (include/mpdata_hip.h 3s) at
ncrms=65536 nx=32 nz=28, cold: consecutive calls go to different plans (field sets) with their own tkh and cz, as bench.py
runs its steps, so no call finds its f in the Infinity Cache.  Per call (torch events around a loop of calls on the plans'
stream, after a wake-up: batches of calls until the batch time has stopped falling, i.e. two consecutive batches agree
within 3 %; the least of three batches, and the spread of those three):
  vdiffuse      : Plan.vdiffuse, the whole plan, with sb and st (the ir kernel included)
  block64       : a block of 64 instances in the middle of the plan (odd sl0)
and four yardsticks in the same process, all of them code of the parent commit:
  round_trip    : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                  without the caller's own kernel
  vsolve        : Plan.vsolve -- the same sweep, no per-cell field, no divides in the hot kernel
  sediment      : Plan.sediment -- the same algorithmic bytes: f read and written once, one per-cell field read once
  diffuse       : Plan.diffuse, the full 3l
and from them the ratios and GB/s against the algorithmic bytes of the call: the interior of f read once and written once
and the interior of tkh read once, (2 T + 1) nx nzm ncrms reals for T tracers.  With --tracers T the call, the round trip
and vsolve on plans of T tracers as well; with --tall-plain NZ the same at --tall-ncrms instances and NZ <= 238 levels.  The
result of one call is checked against a Thomas solve in torch float64 on the exported copies (to rounding).  Needs no
oracle and no reference tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/vdiffuse_bench.py [--steps K] [--sets N] [--json PATH] [--f32] [--tracers 25] [--tall-plain 238]"""
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
ap.add_argument("--ncrms", type=int, default=65536)
ap.add_argument("--nx", type=int, default=32)
ap.add_argument("--nz", type=int, default=28)
ap.add_argument("--json", default=None)
ap.add_argument("--f32", action="store_true", help="fp32 as well")
ap.add_argument("--tracers", type=int, default=0, help="plans of this many tracers as well (0: none)")
ap.add_argument("--tall-plain", type=int, default=0, help="a plain plan of this many levels (<= 238) as well (0: none)")
ap.add_argument("--tall-ncrms", type=int, default=4096)
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler): vdiffuse, vsolve, ...")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"shape": [a.ncrms, a.nx, a.nz], "steps": a.steps, "sets": a.sets, "device": torch.cuda.get_device_name(0)}


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed(fn, steps):
    """-> (the least of three batches, (max - min) / min of the three)"""
    prev = loop_ms(fn, steps)
    for _ in range(8):            # wake-up: until the batch time has stopped falling
        cur = loop_ms(fn, steps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    t = [loop_ms(fn, steps) for _ in range(3)]
    return min(t), (max(t) - min(t)) / min(t)


def measure(tag, tdt, eb, ncrms, nx, nz, T, sets, steps, yardsticks):
    nzm = nz - 1
    sh = M.shapes(ncrms, nx, nz, T)
    dsh = M.vdiffuse_shapes(ncrms, nx, nz)
    vsh = M.vsolve_shapes(ncrms, nz)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda shape, lo, hi: torch.rand(shape, generator=g, device=dev, dtype=torch.float64).mul_(hi - lo).add_(lo).to(tdt)
    plans, cs, vs = [], [], []
    ftmp = torch.empty(sh["f"], dtype=tdt, device=dev)
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and p.level_windows == 1
        p.set_stream()
        p.set_timing(False)
        M.fill_synthetic(ftmp, "f", 100 + s, 1)
        p.import_device(f=ftmp)
        ra = {k: rnd(sh[k], 0.5, 1.0) for k in ("rho", "adz")}
        p.import_device(**ra)
        if s == 0:
            rx, ax = ra["rho"], ra["adz"]
        plans.append(p)
        # tkh in [0, 1) with a third of the cells zero, cz in [0, 2): off-diagonals up to 16; row sums 1, so hundreds of
        # timed calls on one field stay within what they started from
        tkh = rnd(dsh["tkh"], 0.0, 1.0)
        tkh.mul_((rnd(dsh["tkh"], 0.0, 1.0) > 1.0 / 3).to(tdt))
        cs.append((tkh, rnd(dsh["cz"], 0.0, 2.0), rnd(dsh["sb"], -1.0 / 64, 1.0 / 64), rnd(dsh["st"], -1.0 / 64, 1.0 / 64)))
        lo, up = rnd(vsh["lo"], -0.4, 0.0), rnd(vsh["up"], -0.4, 0.0)
        vs.append((lo, (1.0 - lo.double() - up.double()).to(tdt), up))
    del ftmp
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    b0 = ncrms // 2 - 7
    bc = tuple(t[..., b0:b0 + 64].contiguous() for t in cs[0])
    torch.cuda.synchronize()
    n = len(plans)
    cells = float(nzm) * ncrms * nx * eb                 # bytes of one interior field
    alg = cells * (2 * T + 1)                            # f read and written, tkh read
    res = {"shape": [ncrms, nx, nz], "tracers": T, "algorithmic_bytes": alg, "vsolve_bytes": cells * 2 * T,
           "round_trip_bytes": cells * 4 * T * (nx + 6) / nx}

    def round_trip(i):
        plans[i % n].export_device(f=fx)
        plans[i % n].import_device(f=fx)

    # the check first (the timed calls go on changing the same fields): one call against a Thomas solve in float64
    if T == 1:
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        f0 = fx.clone().double()                          # (nzm, nx+6, ncrms)
        plans[0].vdiffuse(*cs[0])
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        tkh, cz, sb, st = (t.double() for t in cs[0])
        ir = (1.0 / (rx.double() * ax.double()))[:, None, :]             # (nzm, 1, ncrms)
        e = torch.zeros((nzm + 1, nx, ncrms), dtype=torch.float64, device=dev)
        e[1:nzm] = cz[:nzm - 1, None, :] * (tkh[:-1, 1:nx + 1] + tkh[1:, 1:nx + 1])
        av, cv = e[:-1] * ir, e[1:] * ir
        di = 1.0 + av + cv
        y = f0[:, 3:nx + 3].clone()
        y[0] += sb * ir[0]
        y[nzm - 1] -= st * ir[nzm - 1]
        gk = torch.zeros_like(di)
        pk = 1.0 / di[0]
        y[0] *= pk
        gk[0] = cv[0] * pk
        for k in range(1, nzm):
            pk = 1.0 / (di[k] - av[k] * gk[k - 1])
            gk[k] = cv[k] * pk
            y[k] = (y[k] + av[k] * y[k - 1]) * pk
        for k in range(nzm - 2, -1, -1):
            y[k] += gk[k] * y[k + 1]
        want = f0.clone()
        want[:, 3:nx + 3] = y
        eps = 2.3e-16 if eb == 8 else 1.2e-7
        err = float((fx.double() - want).abs().max() / f0.abs().max())
        assert err < 64 * eps, (tag, err)
        res["check_err_over_eps"] = err / eps
        del f0, y, gk, want, tkh, cz, sb, st, ir, e, av, cv, di
        torch.cuda.empty_cache()

    runs = {
        "vdiffuse": lambda i: plans[i % n].vdiffuse(*cs[i % n], ntracers=T),
        "block64": lambda i: plans[i % n].vdiffuse(*bc, sl0=b0, n=64, ntracers=T),
        "round_trip": round_trip,
        "vsolve": lambda i: plans[i % n].vsolve(*vs[i % n], ntracers=T),
    }
    if yardsticks:
        wp = rnd(M.sediment_shapes(ncrms, nx, nz)["wp"], 0.0, 0.1)
        cx, czx = rnd(dsh["cz"], 1.0 / 32, 1.0 / 16), rnd(dsh["cz"], 1.0 / 128, 1.0 / 64)
        runs["sediment"] = lambda i: plans[i % n].sediment(wp)
        runs["diffuse"] = lambda i: plans[i % n].diffuse(cs[i % n][0], cx, czx)
    if a.only:
        res[a.only + "_ms"], _ = timed(runs[a.only], steps)
        print(f"{tag:7s}: {a.only} {res[a.only + '_ms']:.4f} ms", flush=True)
    else:
        for k, fn in runs.items():
            res[k + "_ms"], res[k + "_spread"] = timed(fn, steps)
        res["vdiffuse_ms_again"], _ = timed(runs["vdiffuse"], steps)
        for k in runs:
            if k not in ("vdiffuse", "block64"):
                res["ratio_vdiffuse_over_" + k] = res["vdiffuse_ms"] / res[k + "_ms"]
        res["vdiffuse_gbs"] = alg / res["vdiffuse_ms"] / 1e6
        res["vsolve_gbs"] = res["vsolve_bytes"] / res["vsolve_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        line = (f"{tag:9s}: vdiffuse {res['vdiffuse_ms']:.4f} ms ({res['vdiffuse_gbs']:.0f} GB/s, spread {100 * res['vdiffuse_spread']:.1f} %, "
                f"again {res['vdiffuse_ms_again']:.4f})  block of 64 {res['block64_ms']:.4f}  export + import of f "
                f"{res['round_trip_ms']:.4f} (x {res['ratio_vdiffuse_over_round_trip']:.3f})  vsolve {res['vsolve_ms']:.4f} "
                f"(x {res['ratio_vdiffuse_over_vsolve']:.3f})")
        if yardsticks:
            line += (f"  sediment {res['sediment_ms']:.4f} (x {res['ratio_vdiffuse_over_sediment']:.3f})  diffuse {res['diffuse_ms']:.4f} "
                     f"(x {res['ratio_vdiffuse_over_diffuse']:.3f})")
        print(line, flush=True)
    for p in plans:
        p.close()
    del plans, cs, vs, fx
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
kinds = [("f64", torch.float64, 8)] + ([("f32", torch.float32, 4)] if a.f32 else [])
for name, tdt, eb in kinds:
    measure(name + "_t1", tdt, eb, a.ncrms, a.nx, a.nz, 1, a.sets, a.steps, True)
if a.tracers:
    for name, tdt, eb in kinds:
        measure(f"{name}_t{a.tracers}", tdt, eb, a.ncrms, a.nx, a.nz, a.tracers, 2, max(a.steps // 5, 4), False)
if a.tall_plain:
    for name, tdt, eb in kinds:
        measure(f"{name}_nz{a.tall_plain}", tdt, eb, a.tall_ncrms, a.nx, a.tall_plain, 1, min(a.sets, 3), a.steps, False)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
