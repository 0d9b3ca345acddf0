"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases(dtype="f64"):
    """Fixtures of one precision ("f64": the reference as shipped; "f32": its fp32 build)."""
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as fh:
        return [c for c in json.load(fh)["cases"] if c.get("dtype", "f64") == dtype]


def regime_cases(dtype="f64"):
    """Value-regime fixtures (manifest key "regimes", oracle/regimes.py) of one precision."""
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as fh:
        return [c for c in json.load(fh).get("regimes", []) if c["dtype"] == dtype]


def load_golden(case):
    z = np.load(os.path.join(GOLDEN_DIR, case["name"] + ".npz"))
    return np.asfortranarray(z["f"]), np.asfortranarray(z["flux"])


def to_dev(a, device="cuda:0"):
    """Fortran-ordered numpy array -> torch tensor with reversed axes (same bytes)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(device)


def to_host(t):
    """Inverse of to_dev."""
    return np.asfortranarray(t.cpu().numpy().T)


def run_hip(M, inp, device="cuda:0"):
    """Device-resident HIP call on a dict of numpy inputs; returns (f, flux) numpy."""
    import torch
    d = {k: to_dev(v, device) for k, v in inp.items()}
    M.advect_scalar2D(d["f"], d["u"], d["w"], d["rho"], d["rhow"], d["flux"], d["adz"])
    torch.cuda.synchronize()
    return to_host(d["f"]), to_host(d["flux"])


def max_abs(a, b):
    return float(np.max(np.abs(a - b)))


def bits(a):
    """the bit patterns of a: the unsigned integers of its item size"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def bit_mismatches(a, b):
    """Indices where a and b differ as bit patterns (so +0.0 != -0.0, and NaNs compare by payload)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    ui = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return np.nonzero(a.view(ui) != b.view(ui))


def assert_bitwise(a, b, what=""):
    """a and b are equal bit pattern for bit pattern.  On failure: the mismatch count, the first index,
    max|d| and whether every mismatch is a (+0, -0) pair."""
    a, b = np.asarray(a), np.asarray(b)
    bad = bit_mismatches(np.ascontiguousarray(a), np.ascontiguousarray(b))
    n = len(bad[0])
    if n:
        ia, ib = np.ascontiguousarray(a)[bad], np.ascontiguousarray(b)[bad]
        signed_zero_only = bool(np.all((ia == 0) & (ib == 0)))
        first = tuple(int(x[0]) for x in bad)
        d = float(np.max(np.abs(ia.astype(np.float64) - ib.astype(np.float64))))
        raise AssertionError(f"{what}: {n} of {a.size} elements differ in bit pattern; first at {first} "
                             f"({ia[0]!r} vs {ib[0]!r}); max|d| = {d:.3e}; "
                             f"{'every mismatch is a +0/-0 pair' if signed_zero_only else 'not only signed zeros'}")
