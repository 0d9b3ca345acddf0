#!/usr/bin/env python3
"""tests/golden/make_golden.py -- regenerate the golden vectors.

Each fixture is the OUTPUT (f, flux) of the reference Fortran program itself
(built from /root/reference by oracle/build_ref.py, `amdflang -O3
-ffp-contract=off`) on inputs produced by this repo's seeded generator
(oracle/oracle.py:make_inputs).  Inputs are not stored: they are regenerated
from (shape, seed, dist).  Only data is committed (npz + manifest.json); no
reference source text.  Runs in the build container only (needs
/root/reference + amdflang).

    python tests/golden/make_golden.py             # everything
    python tests/golden/make_golden.py --regimes   # only the value-regime fixtures (manifest key "regimes")
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import bwk as B  # noqa: E402
from oracle import nlk as N  # noqa: E402
from oracle import regimes as RG  # noqa: E402

# (ncrms, nx, nz, seed, dist)
CASES = [
    (3, 8, 6, 100, O.DIST_CONDITIONED),
    (3, 8, 6, 100, O.DIST_RAW),
    (3, 8, 6, 100, O.DIST_RAW_SIGNED),
    (8, 32, 28, 100, O.DIST_CONDITIONED),
    (8, 32, 28, 7, O.DIST_RAW_SIGNED),
    (64, 32, 28, 100, O.DIST_CONDITIONED),   # BASELINE.json configs[0]
    (64, 32, 28, 100, O.DIST_RAW),           # ... with the reference's U[0,1) law
    (48, 32, 58, 100, O.DIST_RAW),           # the reference's shipped size (:7-9)
]


# fp32 build of the reference (rp = IEEE single; see oracle/build_ref.py, edit 4): pins the
# fp32 build of the oracle (mpdata_oracle.c with -DMPDATA_ORACLE_F32)
CASES_F32 = [
    (3, 8, 6, 100, O.DIST_CONDITIONED),
    (3, 8, 6, 100, O.DIST_RAW_SIGNED),
    (8, 32, 28, 100, O.DIST_CONDITIONED),
    (64, 32, 28, 100, O.DIST_RAW),
]


# value regimes (oracle/regimes.py) through the reference, fp64 and fp32: every regime at 8 x 32 x 28, a few at
# 3 x 8 x 6.  They pin the oracle where the limiter's eps matters (the fp32 eps included, which the unit-scale
# cases above cannot see) and the sign of zero; kept apart from "cases" (those are rebuilt from (shape, seed, dist)).
REGIME_SHAPES = [((8, 32, 28), RG.REGIMES),
                 ((3, 8, 6), ("scaled_m30", "sparse", "fronts", "signed_zero", "f32_tiny"))]
REGIME_SEED = 100


def regime_name(regime, ncrms, nx, nz, seed, f32=False):
    return f"regime_{regime}_{ncrms}x{nx}x{nz}_seed{seed}" + ("_f32" if f32 else "")


def make_regimes():
    """Run the reference on every regime case; write the .npz fixtures, return the manifest entries."""
    out = []
    for (ncrms, nx, nz), names in REGIME_SHAPES:
        for f32 in (False, True):
            dt = np.float32 if f32 else np.float64
            build_ref.build(ncrms, nx, nz, f32=f32)
            for regime in names:
                if regime not in RG.regimes_for(dt):
                    continue
                inp = RG.make(regime, ncrms, nx, nz, seed=REGIME_SEED, dtype=dt)
                f, flux, _ = O.run_reference(inp)
                name = regime_name(regime, ncrms, nx, nz, REGIME_SEED, f32)
                np.savez(os.path.join(HERE, name + ".npz"), f=f, flux=flux)
                out.append({
                    "name": name, "regime": regime, "ncrms": ncrms, "nx": nx, "nz": nz, "seed": REGIME_SEED,
                    "dtype": "f32" if f32 else "f64",
                    "f_sha256": hashlib.sha256(f.tobytes(order="F")).hexdigest(),
                    "flux_sha256": hashlib.sha256(flux.tobytes(order="F")).hexdigest(),
                    "inputs_sha256": hashlib.sha256(b"".join(
                        inp[k].tobytes(order="F") for k in ("adz", "f", "u", "w", "rho", "rhow", "flux")
                    )).hexdigest(),
                    "f_min": float(f.min()), "f_max": float(f.max())})
                print(name, f.shape, flux.shape)
    return out


NLK_SAMPLE_EDGES, NLK_SAMPLE_SEED = 16, 7


def nlk_edge_sample(inp, ref, nedges, seed):
    """A fixed, seeded sample of the edges of one reference run of the third mini-app: the edges' own
    arrays, the cells they gather (renumbered 1..n in ascending order of their original numbers) and
    the edges' refFlx columns.  An edge's flux depends on nothing else, so the oracle on the sample
    reproduces those columns."""
    edges = np.sort(np.random.default_rng(seed).choice(ref.shape[1], nedges, replace=False))
    adv = inp["advCellsForEdge"][:, edges]
    cells = np.unique(np.concatenate([adv[:n, j] for j, n in enumerate(inp["nAdvCellsForEdge"][edges])]))
    renum = np.zeros(inp["tracerCur"].shape[1] + 1, np.int32)
    renum[cells] = np.arange(1, len(cells) + 1, dtype=np.int32)
    out = {"nAdvCellsForEdge": inp["nAdvCellsForEdge"][edges], "advCellsForEdge": renum[adv],
           "minLevelCell": inp["minLevelCell"][cells - 1], "maxLevelCell": inp["maxLevelCell"][cells - 1],
           "tracerCur": inp["tracerCur"][:, cells - 1]}
    for k in ("normalThicknessFlux", "advMaskHighOrder", "advCoefs", "advCoefs3rd"):
        out[k] = inp[k][:, edges]
    out = {k: np.asfortranarray(v) for k, v in out.items()}
    out.update(coef3rdOrder=inp["coef3rdOrder"], nVertLevels=inp["nVertLevels"], edges=edges, cells=cells)
    return out, np.asfortranarray(ref[:, edges])


def case_name(ncrms, nx, nz, seed, dist, f32=False):
    return f"ref_{ncrms}x{nx}x{nz}_seed{seed}_dist{dist}" + ("_f32" if f32 else "")


def main():
    if "--regimes" in sys.argv[1:]:
        with open(os.path.join(HERE, "manifest.json")) as fh:
            manifest = json.load(fh)
        manifest["regimes"] = make_regimes()
        with open(os.path.join(HERE, "manifest.json"), "w") as fh:
            json.dump(manifest, fh, indent=1)
        return
    manifest = {"generator": "tests/golden/make_golden.py",
                "reference": "mmf-mpdata-tracer/advect_scalar2D_pushncols_openacc.F90 "
                             "(advect_scalar2D_cpu, :477-642)",
                "compiler": "amdflang -O3 -ffp-contract=off",
                "cases": []}
    for (ncrms, nx, nz, seed, dist, f32) in [c + (False,) for c in CASES] + [c + (True,) for c in CASES_F32]:
        build_ref.build(ncrms, nx, nz, f32=f32)
        inp = O.make_inputs(ncrms, nx, nz, seed=seed, dist=dist,
                            dtype=np.float32 if f32 else np.float64)
        f, flux, _ = O.run_reference(inp)
        name = case_name(ncrms, nx, nz, seed, dist, f32)
        path = os.path.join(HERE, name + ".npz")
        np.savez(path, f=f, flux=flux)
        manifest["cases"].append({
            "name": name, "ncrms": ncrms, "nx": nx, "nz": nz, "seed": seed, "dist": dist,
            "dtype": "f32" if f32 else "f64",
            "f_sha256": hashlib.sha256(f.tobytes(order="F")).hexdigest(),
            "flux_sha256": hashlib.sha256(flux.tobytes(order="F")).hexdigest(),
            "inputs_sha256": hashlib.sha256(b"".join(
                inp[k].tobytes(order="F") for k in ("adz", "f", "u", "w", "rho", "rhow", "flux")
            )).hexdigest(),
            "f_min": float(f.min()), "f_max": float(f.max()),
        })
        print(name, f.shape, flux.shape)
    # second mini-app (atmosphere/biharmonic_wk_kernel.F90): the reference program generates
    # its own inputs (a portable LCG); fixtures = the qtens its CPU routine returns.  One
    # element in full, the shipped size (16 elements) as a sha256.
    manifest["bwk"] = {"reference": "atmosphere/biharmonic_wk_kernel.F90 (biharmonic_wk_scalar CPU, :186-200; "
                                    "inputs: initialize_data :48-58)", "cases": []}
    for nelemd, keep in ((1, True), (2, False), (16, False)):
        build_ref.build_bwk(nelemd)
        inp, out, _ = B.run_reference(nelemd)
        name = f"bwk_ref_ne{nelemd}"
        if keep:
            np.savez(os.path.join(HERE, name + ".npz"), qtens=out)
        manifest["bwk"]["cases"].append({
            "name": name, "nelemd": nelemd, "nlev": B.NLEV, "qsize": B.QSIZE, "stored": keep,
            "qtens_out_sha256": hashlib.sha256(out.tobytes(order="F")).hexdigest(),
            "inputs_sha256": hashlib.sha256(b"".join(inp[k].tobytes(order="F") for k in ("dvv", "elem", "qtens"))).hexdigest(),
            "out_min": float(out.min()), "out_max": float(out.max())})
        print(name, out.shape)
    # third mini-app (nested_loops/nested.F90): the program's inputs depend on the compiler's
    # random_number, so the reference is fed a seeded stream (oracle/build_ref.py --nlk) and the
    # fixture keeps the inputs the PROGRAM built from it together with its refFlx.
    build_ref.build_nlk()
    manifest["nlk"] = {"reference": "nested_loops/nested.F90 (CPU reference loop :123-157 -> refFlx)", "cases": []}
    for name, shape, seed, keep in (("nlk_ref_small", (64, 20, 12, 4), 5, True),
                                    ("nlk_ref_nml", (25600, 2800, 100, 10), 5, False)):
        inp, ref = N.run_reference(*shape, seed=seed)
        if keep:
            np.savez(os.path.join(HERE, name + ".npz"), refFlx=ref, **{k: v for k, v in inp.items()})
        manifest["nlk"]["cases"].append({
            "name": name, "nEdges": shape[0], "nCells": shape[1], "nVertLevels": shape[2], "nAdv": shape[3],
            "seed": seed, "stored": keep, "refFlx_sha256": hashlib.sha256(ref.tobytes(order="F")).hexdigest()})
        print(name, ref.shape)
        if name == "nlk_ref_nml":   # the shipped size is too large to store: a seeded sample of its edges
            sname = name + "_sample"
            sinp, sref = nlk_edge_sample(inp, ref, NLK_SAMPLE_EDGES, NLK_SAMPLE_SEED)
            np.savez(os.path.join(HERE, sname + ".npz"), refFlx=sref, **sinp)
            manifest["nlk"]["cases"].append({
                "name": sname, "of": name, "nEdges": NLK_SAMPLE_EDGES, "nCells": int(sinp["tracerCur"].shape[1]),
                "sample_seed": NLK_SAMPLE_SEED, "stored": True,
                "refFlx_sha256": hashlib.sha256(sref.tobytes(order="F")).hexdigest()})
            print(sname, sref.shape)
    manifest["regimes"] = make_regimes()
    with open(os.path.join(HERE, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)


if __name__ == "__main__":
    main()
