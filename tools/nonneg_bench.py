#!/usr/bin/env python3
"""Time of the conservative per-level non-negativity fixer of a resident plan's tracers (include/mpdata_hip.h 3x), cold, at
ncrms=65536 nx=32 nz=28 with one tracer and with 25, and at ncrms=4096 nx=32 nz=300 (a windowed plan), fp64 and fp32.  The
call changes what it acts on -- a fixed field has nothing left to fix --, so a measurement is a ROUND: every plan (field
set) takes its field again by an import of f, untimed; then one call goes to each plan, plan after plan, between two torch
events on the plans' stream.  No call finds its f in the Infinity Cache: the imports and the calls on the other plans have
gone over it (the 25-tracer plans are one set: a call moves more bytes than any cache holds).  Rounds repeat until the
round time has stopped falling, i.e. two consecutive rounds agree within 3 %; then the minimum, the median AND the maximum
of five rounds, the run-to-run spread.  Three fields:
  nonneg_clean   : (a) no negative cell: every row is read, none is stored
  nonneg_all     : (b) every row in need: column 1 of every row is negative, the row sum positive -- every row is scaled
  nonneg_mix     : (c) the mix of tests/nonneg_model.py: on five of every seven levels of an instance a planted row
                   (non-negative with a -0.0, wholly negative, shifted by -0.6, scaled by 1e-3 with one cell at -1e-9,
                   non-negative), the others uniform in [-0.15, 1)
  nonneg_all_out : (b) with sum and nneg written
and three yardsticks in the same process and by the same rounds, all of them calls that exist without 3x, on field (b):
  round_trip  : Plan.export_device + Plan.import_device of f alone -- the route a caller had before the call existed,
                without the caller's own two-pass kernel
  level_stats : Plan.level_stats (sum only) -- the same bytes from HBM as (a), no store
  relax_mean  : Plan.relax without a target, c != 0 on every level -- the same bytes as (b) and one divide per row
and from them the ratios and GB/s against the bytes each call moves: nonneg (a) and level_stats nx nzm ncrms reals (the
interior of f read once), nonneg (b) and relax twice that (read once and written once; a second read of the RE-READ form
is not counted), the round trip 4 (nx + 6) columns.  The result of one call on fields (b) and (c) is checked against torch
on the exported copies (to rounding: torch sums in another order), (a) bit for bit.  Needs no oracle and no reference
tree.  Prints one line per measurement and, with --json PATH, writes them all there.
usage: python tools/nonneg_bench.py [--sets N] [--json PATH] [--no-f32] [--no-tall] [--no-tracers] [--only NAME]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import codesign_kernels_amd as M

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--shape", type=int, nargs=3, default=[65536, 32, 28], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tall-shape", type=int, nargs=3, default=[4096, 32, 300], metavar=("NCRMS", "NX", "NZ"))
ap.add_argument("--tracers", type=int, default=25, help="tracers of the many-tracer case")
ap.add_argument("--json", default=None)
ap.add_argument("--no-f32", action="store_true", help="fp64 only")
ap.add_argument("--no-tall", action="store_true", help="no windowed plan")
ap.add_argument("--no-tracers", action="store_true", help="no many-tracer case")
ap.add_argument("--only", default=None, help="time this one measurement alone (for a profiler), e.g. nonneg_all")
a = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"sets": a.sets, "device": torch.cuda.get_device_name(0), "library": os.path.basename(M.lib_path())}


def make_fields(shape, T, tdt):
    """(clean, all, mix): f ([T,] nzm, nx+6, ncrms) of the three kinds"""
    ncrms, nx, nz = shape
    nzm = nz - 1
    g = torch.Generator(device=dev).manual_seed(11)
    sh = M.shapes(ncrms, nx, nz, T)["f"]
    base = torch.rand(sh, generator=g, device=dev, dtype=torch.float64).mul_(1.15).sub_(0.15)       # [-0.15, 1)
    clean = base.abs().to(tdt)
    every = base.abs()
    every[..., 3, :] = -0.1                                   # column 1: every row in need, its sum positive for nx > 1
    every = every.to(tdt)
    kind = (torch.arange(nzm, device=dev)[:, None] + torch.arange(ncrms, device=dev)[None, :]) % 7       # (nzm, ncrms)
    k = kind[:, None, :]                                      # over the columns
    mix = base.clone()
    mix = torch.where((k == 0) | (k == 4), mix.abs(), mix)
    mix = torch.where(k == 1, -mix.abs() - 1e-3, mix)
    mix = torch.where(k == 2, mix - 0.6, mix)
    mix = torch.where(k == 3, mix.abs() * 1e-3, mix)
    mix[..., 4, :] = torch.where(kind == 3, torch.full_like(mix[..., 4, :], -1e-9), mix[..., 4, :])
    mix[..., 5, :] = torch.where(kind == 0, torch.full_like(mix[..., 5, :], -0.0), mix[..., 5, :])
    return clean, every, mix.to(tdt)


def model(f0, nx):
    """torch, in double: (f_new, sum, nneg) of f0 ([T,] nzm, nx+6, ncrms)"""
    fi = f0[..., 3:nx + 3, :]
    s = fi.sum(dim=-2)
    y = fi.clamp(min=0)
    p = y.sum(dim=-2)
    c = (fi < 0).sum(dim=-2).double()
    r = torch.where(s > 0, s / p.clamp(min=1e-300), torch.zeros_like(s))
    want = f0.clone()
    want[..., 3:nx + 3, :] = torch.where((c > 0).unsqueeze(-2), y * r.unsqueeze(-2), fi)
    return want, s, c


def measure(tag, shape, T, tdt, eb, sets, tall):
    ncrms, nx, nz = shape
    nzm = nz - 1
    M.set_tall_columns(int(tall))
    sh = M.shapes(ncrms, nx, nz, T)
    nsh = M.nonneg_shapes(ncrms, nx, nz, T if T > 1 else None)
    rsh = M.relax_shapes(ncrms, nx, nz, T if T > 1 else None)
    fields = dict(zip(("clean", "all", "mix"), make_fields(shape, T, tdt)))
    ssum = torch.empty(nsh["sum"], dtype=tdt, device=dev)
    nneg = torch.empty(nsh["nneg"], dtype=tdt, device=dev)
    c = torch.full(rsh["c"], 0.01, dtype=tdt, device=dev)     # != 0 on every level: every level is loaded and stored
    plans = []
    for s in range(sets):
        p = M.Plan(ncrms, nx, nz, T, dtype={8: "float64", 4: "float32"}[eb])
        assert p.layout == M.LAYOUT_WAVEMAJOR and (p.level_windows > 1) == tall
        p.set_stream()
        p.set_timing(False)
        p.import_device(f=fields["clean"])
        plans.append(p)
    fx = torch.empty(sh["f"], dtype=tdt, device=dev)
    torch.cuda.synchronize()
    n = len(plans)
    col = float(nzm) * ncrms * eb * T                        # bytes of one column of all instances and tracers
    res = {"shape": [ncrms, nx, nz], "tracers": T, "level_windows": int(plans[0].level_windows), "read_bytes": col * nx,
           "read_write_bytes": col * 2 * nx, "round_trip_bytes": col * 4 * (nx + 6)}

    # the check first: one call on each field against torch on the exported copies (one tracer: the many-tracer case runs
    # the same kernel, and its copies in double would not fit next to the fields)
    eps = 2.3e-16 if eb == 8 else 1.2e-7
    shares = {}
    for name, f in fields.items() if T == 1 else ():
        plans[0].import_device(f=f)
        plans[0].nonneg(ssum, nneg)
        plans[0].export_device(f=fx)
        torch.cuda.synchronize()
        f0 = f.double()
        want, s, cn = model(f0, nx)
        shares[name] = float((cn > 0).double().mean())
        assert torch.equal(nneg.double(), cn), (tag, name, "nneg")
        scale = float(f0.abs().max()) * nx
        assert float((ssum.double() - s).abs().max()) < nx * eps * scale, (tag, name, "sum")
        assert float((fx.double() - want).abs().max()) < (2 * nx + 8) * eps * scale, (tag, name, "f")
        assert float(torch.where((cn > 0).unsqueeze(-2), fx[..., 3:nx + 3, :].double(), torch.zeros_like(want[..., 3:nx + 3, :])).min()) >= 0
        assert torch.equal(fx[..., :3, :], f[..., :3, :]) and torch.equal(fx[..., nx + 3:, :], f[..., nx + 3:, :]), "halo columns changed"
        if name == "clean":
            assert torch.equal(fx.view(torch.uint8), f.view(torch.uint8)), "a clean field changed"
        del f0, want, s, cn
    if shares:
        assert shares["clean"] == 0 and shares["all"] == 1 and 0.3 < shares["mix"] < 0.9, shares
        res["rows_in_need"] = shares
    torch.cuda.empty_cache()

    def rounds(field, fn):
        """-> (min, median, max) ms per call over five rounds behind the wake-up"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def one():
            for p in plans:
                p.import_device(f=fields[field])
            torch.cuda.synchronize()
            e0.record()
            for p in plans:
                fn(p)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n

        prev = one()
        for _ in range(8):        # wake-up: until the round time has stopped falling
            cur = one()
            if abs(cur - prev) <= 0.03 * prev:
                break
            prev = cur
        t = [one() for _ in range(5)]
        return min(t), statistics.median(t), max(t)

    def round_trip(p):
        p.export_device(f=fx)
        p.import_device(f=fx)

    runs = {
        "nonneg_clean": ("clean", lambda p: p.nonneg(ntracers=T)),
        "nonneg_all": ("all", lambda p: p.nonneg(ntracers=T)),
        "nonneg_mix": ("mix", lambda p: p.nonneg(ntracers=T)),
        "nonneg_all_out": ("all", lambda p: p.nonneg(ssum, nneg)),
        "round_trip": ("all", round_trip),
        "level_stats": ("all", lambda p: p.level_stats(sum=ssum)),
        "relax_mean": ("all", lambda p: p.relax(c, ntracers=T)),
    }
    for k, (field, fn) in runs.items():
        if a.only and k != a.only:
            continue
        res[k + "_ms"], res[k + "_ms_median"], res[k + "_ms_max"] = rounds(field, fn)
        print(f"{tag:12s}: {k:15s} {res[k + '_ms']:.4f} ms (median {res[k + '_ms_median']:.4f}, max {res[k + '_ms_max']:.4f})", flush=True)
    if not a.only:
        res["nonneg_clean_ms_again"], _, _ = rounds(*runs["nonneg_clean"])
        res["nonneg_all_ms_again"], _, _ = rounds(*runs["nonneg_all"])
        for r in ("nonneg_clean", "nonneg_all", "nonneg_mix"):
            for k in ("round_trip", "level_stats", "relax_mean"):
                res[f"ratio_{r}_over_{k}"] = res[r + "_ms"] / res[k + "_ms"]
        res["nonneg_clean_gbs"] = res["read_bytes"] / res["nonneg_clean_ms"] / 1e6
        res["level_stats_gbs"] = res["read_bytes"] / res["level_stats_ms"] / 1e6
        res["nonneg_all_gbs"] = res["read_write_bytes"] / res["nonneg_all_ms"] / 1e6
        res["relax_mean_gbs"] = res["read_write_bytes"] / res["relax_mean_ms"] / 1e6
        res["round_trip_gbs"] = res["round_trip_bytes"] / res["round_trip_ms"] / 1e6
        print(f"{tag:12s}: (a) clean {res['nonneg_clean_ms']:.4f} ms (again {res['nonneg_clean_ms_again']:.4f}; {res['nonneg_clean_gbs']:.0f} GB/s) "
              f"= {res['ratio_nonneg_clean_over_level_stats']:.3f} x level_stats ({res['level_stats_ms']:.4f}, {res['level_stats_gbs']:.0f} GB/s)  "
              f"(b) all {res['nonneg_all_ms']:.4f} (again {res['nonneg_all_ms_again']:.4f}; {res['nonneg_all_gbs']:.0f} GB/s) = "
              f"{res['ratio_nonneg_all_over_relax_mean']:.3f} x relax to the mean ({res['relax_mean_ms']:.4f}, {res['relax_mean_gbs']:.0f} GB/s)  "
              f"(c) mix {res['nonneg_mix_ms']:.4f}  export + import {res['round_trip_ms']:.4f} ({res['round_trip_gbs']:.0f} GB/s): "
              f"(a) {res['ratio_nonneg_clean_over_round_trip']:.3f} x  (b) {res['ratio_nonneg_all_over_round_trip']:.3f} x  "
              f"(c) {res['ratio_nonneg_mix_over_round_trip']:.3f} x", flush=True)
    for p in plans:
        p.close()
    del plans, fx, fields
    torch.cuda.empty_cache()
    out[tag] = res


M.set_variant(M.VARIANT_FAST)
prec = [("f64", torch.float64, 8)] + ([] if a.no_f32 else [("f32", torch.float32, 4)])
cases = [(t, tuple(a.shape), 1, tdt, eb, a.sets, False) for t, tdt, eb in prec]
if not a.no_tracers:
    cases += [(f"{t}_{a.tracers}tr", tuple(a.shape), a.tracers, tdt, eb, 1, False) for t, tdt, eb in prec]
if not a.no_tall:
    cases += [(t + "_tall", tuple(a.tall_shape), 1, tdt, eb, a.sets, True) for t, tdt, eb in prec]
for tag, shape, T, tdt, eb, sets, tall in cases:
    measure(tag, shape, T, tdt, eb, sets, tall)
M.set_tall_columns(0)
print(json.dumps(out))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh, indent=1)
