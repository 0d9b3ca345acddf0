"""oracle/bwk.py -- TEST INFRASTRUCTURE: Python face of the CPU oracle of the second
mini-app (atmosphere/biharmonic_wk_kernel.F90).  Wraps
oracle/libbwk_oracle.so (bwk_oracle.c) and oracle/_ref/bwk_ref_ne<N> (the reference program
itself, built by build_ref.py --bwk).  Only tests/, smoke() and bench.py's cpu_baseline leg
import this module."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from oracle.rounding import GAMMA_U, gamma  # noqa: F401  (the bound gamma(PATH_ROUNDINGS) * S, biharmonic_hi below)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbwk_oracle.so")
REF_DIR = os.path.join(HERE, "_ref")
NP, NLEV, QSIZE = 4, 72, 40      # reference :8-10
ELEM_DOUBLES = 144               # Dinv(4,4,2,2) | spheremp(4,4) | tensorVisc(4,4,2,2), reference :23-27

_lib = None


def build_lib(force=False):
    src = os.path.join(HERE, "bwk_oracle.c")
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= os.path.getmtime(src):
        return LIB_PATH
    subprocess.run(["gcc", "-O3", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-o", LIB_PATH, src, "-lm"],
                   check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build_lib()
        L = ctypes.CDLL(LIB_PATH)
        dp = ctypes.POINTER(ctypes.c_double)
        L.bwk_oracle_biharmonic.restype = ctypes.c_int
        L.bwk_oracle_biharmonic.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, dp, dp, dp, ctypes.c_int]
        L.bwk_oracle_init.restype = None
        L.bwk_oracle_init.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, dp, dp, dp]
        _lib = L
    return _lib


def _dp(a):
    assert a.dtype == np.float64 and a.flags["F_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def make_inputs(nelemd, nlev=NLEV, qsize=QSIZE):
    """The reference's own inputs (initialize_data, reference :48-58): dict of Fortran-ordered
    arrays dvv(4,4), elem(144,nelemd), qtens(4,4,nlev,qsize,nelemd)."""
    dvv = np.zeros((NP, NP), order="F")
    elem = np.zeros((ELEM_DOUBLES, nelemd), order="F")
    qtens = np.zeros((NP, NP, nlev, qsize, nelemd), order="F")
    lib().bwk_oracle_init(nelemd, nlev, qsize, _dp(dvv), _dp(elem), _dp(qtens))
    return {"dvv": dvv, "elem": elem, "qtens": qtens}


def random_inputs(nelemd, nlev, qsize, seed):
    """Other data than the reference's LCG (sizes and values the reference never runs)."""
    rng = np.random.default_rng(seed)
    return {"dvv": np.asfortranarray(rng.uniform(-1, 1, (NP, NP))),
            "elem": np.asfortranarray(rng.uniform(-1, 1, (ELEM_DOUBLES, nelemd))),
            "qtens": np.asfortranarray(rng.uniform(-1, 1, (NP, NP, nlev, qsize, nelemd)))}


def biharmonic(inp, nthreads=1):
    """C restatement of biharmonic_wk_scalar (reference :186-200) on a copy of inp['qtens']."""
    q = np.array(inp["qtens"], order="F", copy=True)
    _, _, nlev, qsize, nelemd = q.shape
    rc = lib().bwk_oracle_biharmonic(nelemd, nlev, qsize, _dp(inp["dvv"]), _dp(inp["elem"]), _dp(q), nthreads)
    if rc:
        raise RuntimeError("bwk_oracle_biharmonic failed")
    return q


def ref_exe(nelemd):
    p = os.path.join(REF_DIR, f"bwk_ref_ne{nelemd}")
    return p if os.path.exists(p) else None


def run_reference(nelemd):
    """Run the reference executable; returns (inputs dict as the program generated them, the
    CPU routine's qtens, its 'CPU time' seconds)."""
    exe = ref_exe(nelemd)
    if exe is None:
        raise FileNotFoundError(f"no oracle/_ref/bwk_ref_ne{nelemd}")
    with tempfile.TemporaryDirectory(prefix="bwk_refrun_") as tmp:
        res = subprocess.run([exe], cwd=tmp, check=True, capture_output=True, text=True)
        m = re.search(r"CPU\s+time:\s*([0-9.Ee+-]+)", res.stdout)
        t = float(m.group(1)) if m else float("nan")
        raw = np.fromfile(os.path.join(tmp, "bwk_in.bin"), dtype=np.float64)
        out = np.fromfile(os.path.join(tmp, "bwk_out.bin"), dtype=np.float64)
    shp = (NP, NP, NLEV, QSIZE, nelemd)
    n_el = ELEM_DOUBLES * nelemd
    inp = {"dvv": raw[:16].reshape((NP, NP), order="F").copy(order="F"),
           "elem": raw[16:16 + n_el].reshape((ELEM_DOUBLES, nelemd), order="F").copy(order="F"),
           "qtens": raw[16 + n_el:].reshape(shp, order="F").copy(order="F")}
    return inp, out.reshape(shp, order="F").copy(order="F"), t


def l2norm(a, b):
    """The reference's own metric (reference :69-73)."""
    return float(np.sqrt(np.sum((a - b) ** 2) / np.sum(b ** 2)))


# ------------------------------------------------------------------ a second, independent reference
# Rounded operations on the longest input-to-output path of the reference expression (reference :109-200):
#   gradient_sphere      Dvv*s (1), four additions of the running sum (5), *rrearth (6);
#                        Dinv*v (7), the addition of the two products (8)
#   laplace_sphere_wk    oldgrads*tensorVisc (9), the addition (10)
#   divergence_sphere_wk Dinv*v (11), the addition (12); spheremp*vtemp (13), *Dvv (14), the addition inside
#                        the parentheses (15), *rrearth (16), four subtractions from the running div (20)
# rrearth is the same double in every implementation (the fp32 literal widened), so it carries no error.  Two of
# the 20 (the first addition of each running sum: 0 + x) are exact; that margin covers the np.longdouble
# reference's own error gamma_64(20) * S = 2^-11 gamma_53(20) * S.
PATH_ROUNDINGS = 20


def _laplace_ld(q, dvv, elem, rr):
    """laplace_sphere_wk on q(4,4,nslab,nelemd) in the dtype of its arguments, whole-array einsum form; with
    non-negative arguments and sign=+1 it is the sum S of absolute values of every term"""
    di = elem[0:64].reshape((4, 4, 2, 2, -1), order="F")[:, :, :, :, None, :]     # Dinv(i,j,c,d) -> (i,j,c,d,1,e)
    sp = elem[64:80].reshape((4, 4, -1), order="F")[:, :, None, :]
    tv = elem[80:144].reshape((4, 4, 2, 2, -1), order="F")[:, :, :, :, None, :]
    v1 = np.einsum("il,ijse->ljse", dvv, q) * rr                                   # :121, :124
    v2 = np.einsum("il,jise->jlse", dvv, q) * rr                                   # :122, :125
    ds1 = di[:, :, 0, 0] * v1 + di[:, :, 1, 0] * v2                                # :130
    ds2 = di[:, :, 0, 1] * v1 + di[:, :, 1, 1] * v2                                # :131
    g1 = ds1 * tv[:, :, 0, 0] + ds2 * tv[:, :, 0, 1]                               # :175-176
    g2 = ds1 * tv[:, :, 1, 0] + ds2 * tv[:, :, 1, 1]                               # :177-178
    p1 = sp * (di[:, :, 0, 0] * g1 + di[:, :, 0, 1] * g2)                          # :147, spheremp(j,n)*vtemp(j,n,1)
    p2 = sp * (di[:, :, 1, 0] * g1 + di[:, :, 1, 1] * g2)                          # :148, spheremp(m,j)*vtemp(m,j,2)
    return (np.einsum("jnse,mj->mnse", p1, dvv) + np.einsum("mjse,nj->mnse", p2, dvv)) * rr   # :155-156 (without the sign)


def biharmonic_hi(inp):
    """biharmonic_wk_scalar (reference :109-200) restated in np.longdouble with einsum; shares no code with
    bwk_oracle.c.  Returns (result, S), both shaped like qtens: S is the same computation on |dvv|, |elem|,
    |qtens| with every subtraction turned into an addition, so that any fp64 evaluation `out` of the reference
    expression satisfies |out - result| <= gamma(PATH_ROUNDINGS) * S elementwise."""
    L = np.longdouble
    assert np.finfo(L).nmant >= 63, "np.longdouble is not wider than double here"
    rr = L(np.float64(np.float32(0.00000016666666666666)))                         # reference :14, fp32 literal widened
    shape = inp["qtens"].shape
    q = inp["qtens"].astype(L).reshape((4, 4, shape[2] * shape[3], shape[4]), order="F")
    dvv, elem = inp["dvv"].astype(L), inp["elem"].astype(L)
    hi = -_laplace_ld(q, dvv, elem, rr)
    S = _laplace_ld(np.abs(q), np.abs(dvv), np.abs(elem), rr)
    return hi.reshape(shape, order="F"), S.reshape(shape, order="F")
