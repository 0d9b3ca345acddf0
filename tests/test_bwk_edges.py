"""biharmonic_wk_scalar of libbwk_hip.so (reference atmosphere/biharmonic_wk_kernel.F90:109-200) at the shapes,
placements and value regimes that tests/test_bwk.py leaves open, against TWO references: the C oracle (EXACT is
bit-identical to it) and oracle/bwk.py::biharmonic_hi, an np.longdouble einsum restatement that shares no code with it.

The accuracy bar is derived, not measured: every fp64 evaluation of the reference expression -- any order, with or
without FMA contraction -- satisfies |out - hi| <= gamma(c) * S elementwise, gamma(m) = m u / (1 - m u), u = 2^-53,
c = oracle.bwk.PATH_ROUNDINGS = 20 rounded operations on the longest input-to-output path (counted there, line by
line), S = the same expression on absolute values with every subtraction an addition.  The bound is homogeneous in the
inputs, so it serves every power-of-two scale; where S = 0 it demands a zero.  The sparse regime zeroes 90 % of the
field only (assert_sparse_is_not_vacuous: most results stay non-zero, whole zero slabs give exact zeros)."""
import ctypes
import os

import numpy as np
import pytest

from util import assert_bitwise, to_dev, to_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "codesign-kernels_amd", "libbwk_hip.so")
WORST = {}                                   # (variant, regime) -> (worst |out - hi| / (gamma(c) S), where)
SENTINEL = 0x7FF8DEADBEEF0001                # a NaN payload pattern, compared as 64-bit integers


@pytest.fixture(scope="module")
def B():
    from oracle import bwk
    bwk.build_lib()
    return bwk


def regime_inputs(B, regime, nelemd=3, nlev=9, qsize=5, seed=0):
    rng = np.random.default_rng(seed)
    inp = B.random_inputs(nelemd, nlev, qsize, seed=100 + seed)
    if regime.startswith("2^"):
        s = 2.0 ** int(regime[2:])
        inp = {k: np.asfortranarray(v * s) for k, v in inp.items()}
    elif regime == "sparse":                 # 90 % exact zeros in the field; dvv and elem stay dense (a sparse 4 x 4
        q = inp["qtens"]                     # dvv annihilates every term: zero in, zero out, nothing checked)
        inp["qtens"] = np.asfortranarray(np.where(rng.random(q.shape) < 0.9, 0.0, q))
    elif regime == "negative-zero":
        inp = {k: np.asfortranarray(np.where(rng.random(v.shape) < 0.3, -0.0, v)) for k, v in inp.items()}
        assert all(np.any(np.signbit(v) & (v == 0)) for v in inp.values())
    else:
        assert regime == "unit"
    return inp


REGIMES = ("unit", "2^-30", "2^-10", "2^12", "sparse", "negative-zero")


def assert_sparse_is_not_vacuous(inp, S, out, what):
    """90 % of the field is zero and dvv, elem are dense, yet S is non-zero in more than half of the elements (a slab's
    result vanishes only when all 16 points of the slab do: 0.9^16 = 19 % of the slabs), and the result has exact zeros
    and non-zeros.  A field of a few slabs cannot show the shares: of those only a non-zero S is asked."""
    assert np.all(inp["dvv"] != 0) and np.all(inp["elem"] != 0) and np.any(S != 0) and np.any(out != 0), what
    if out.size >= 16 * 45:
        assert 0.85 < np.mean(inp["qtens"] == 0) < 0.95, what
        assert np.mean(S != 0) > 0.5, f"{what}: S is non-zero in {np.mean(S != 0):.2f} of the elements"
        assert np.any(out == 0) and np.mean(out != 0) > 0.5, f"{what}: {np.mean(out != 0):.2f} of the results are non-zero"


def within_bound(B, out, hi, S, what, key):
    L = np.longdouble
    assert np.all(np.isfinite(out)), what
    err, bound = np.abs(out.astype(L) - hi), L(B.gamma(B.PATH_ROUNDINGS)) * S
    zero = S == 0
    ratio = float(np.max(np.where(zero, L(0), err / np.where(zero, L(1), bound))))
    if ratio > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (ratio, what)
    assert np.all(err <= bound), f"{what}: worst |out - hi| / (gamma({B.PATH_ROUNDINGS}) S) = {ratio:.3f}"


# ------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("regime", REGIMES)
def test_oracle_within_the_derived_bound_of_the_longdouble_reference(B, regime):
    inp = regime_inputs(B, regime)
    hi, S = B.biharmonic_hi(inp)
    assert np.all(S >= np.abs(hi))
    out = B.biharmonic(inp)
    if regime == "sparse":
        assert_sparse_is_not_vacuous(inp, S, out, "oracle sparse")
    within_bound(B, out, hi, S, f"oracle {regime}", ("oracle", regime))


def test_oracle_within_the_derived_bound_on_the_reference_inputs(B):
    inp = B.make_inputs(2)                   # the reference's own LCG data, 72 x 40
    hi, S = B.biharmonic_hi(inp)
    out = B.biharmonic(inp)
    within_bound(B, out, hi, S, "oracle make_inputs", ("oracle", "reference-lcg"))
    assert np.max(np.abs(out.astype(np.longdouble) - hi) / S) > 0      # (two references, not one computed twice)


def test_unaligned_pointers_are_refused_before_any_device_call():
    """a non-null qtens or elem with (p & 31) != 0 -> BWK_EINVAL with the alignment text.  The check precedes every
    device call, so fake non-null integers do; an aligned pair of fakes is never passed."""
    assert os.path.exists(LIB), "libbwk_hip.so is not built (run __graft_entry__.build()): the check cannot run"
    L = ctypes.CDLL(LIB)
    L.bwk_biharmonic_wk_scalar_device.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.bwk_last_error.restype = ctypes.c_char_p
    dvv = 0x30008
    for qtens, elem in [(0x10008, 0x20010), (0x10010, 0x20000), (0x10000, 0x20008), (0x10018, 0x20020), (0x10001, 0x20000)]:
        assert (qtens & 31) or (elem & 31)
        assert L.bwk_biharmonic_wk_scalar_device(2, 3, 4, qtens, dvv, elem, None) == -1, (hex(qtens), hex(elem))
        assert b"32-byte aligned" in L.bwk_last_error()


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available()
    import codesign_kernels_amd.bwk as bwk_hip
    yield bwk_hip
    bwk_hip.set_variant(bwk_hip.VARIANT_EXACT)


def run_hip(K, inp, variant):
    import torch
    K.set_variant(variant)
    d = {k: to_dev(v) for k, v in inp.items()}
    K.biharmonic_wk_scalar(d["elem"], d["qtens"], d["dvv"])
    torch.cuda.synchronize()
    return to_host(d["qtens"])


def check_both(K, B, inp, what, regime, nthreads=1):
    ref = B.biharmonic(inp, nthreads=nthreads)
    hi, S = B.biharmonic_hi(inp)
    outs = {}
    for variant in (0, 1):
        out = run_hip(K, inp, variant)
        if variant == 0:
            assert_bitwise(out, ref, f"{what} exact")
        if regime == "sparse":
            assert_sparse_is_not_vacuous(inp, S, out, f"{what} variant={variant}")
        within_bound(B, out, hi, S, f"{what} variant={variant}", (("exact", "fast")[variant], regime))
        outs[variant] = out
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_c1_accuracy_by_regime(K, B, regime):
    for seed, shape in enumerate([(3, 9, 5), (2, 72, 40), (5, 1, 1)]):
        check_both(K, B, regime_inputs(B, regime, *shape, seed=seed), f"{regime} {shape}", regime)


@pytest.mark.gpu
@pytest.mark.parametrize("nlev,qsize", [(1, 1), (7, 9), (64, 1), (13, 5), (31, 33), (32, 32), (41, 25), (23, 89), (683, 3),
                                        (72, 40), (439, 7)], ids=lambda v: str(v))
def test_c2_slab_counts_at_the_pass_boundaries(K, B, nlev, qsize):
    """nlev*qsize = 1, 63, 64, 65 (one pass of 64 slabs), 1023, 1024, 1025 (16 passes: one workgroup per element),
    2047, 2049, 2880, 16*64*3 + 1 (the workgroup split of launch()); factor pairs with prime nlev (7, 13, 31, 41, 23,
    683, 439)"""
    assert nlev * qsize in (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 2880, 16 * 64 * 3 + 1)
    check_both(K, B, B.random_inputs(2, nlev, qsize, seed=nlev + qsize), f"{nlev}x{qsize}", "shapes", nthreads=2)


@pytest.mark.gpu
@pytest.mark.parametrize("nelemd", [1, 2, 65535])
def test_c2_element_counts_up_to_the_limit(K, B, nelemd):
    """nelemd is the y extent of the launch grid: 65535 is its limit (bwk_hip.h refuses more)"""
    check_both(K, B, B.random_inputs(nelemd, 2, 2, seed=nelemd % 97), f"nelemd={nelemd}", "shapes", nthreads=8)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["exact", "fast"])
def test_c2_qtens_beyond_2_31_doubles(K, B, variant):
    """nelemd = 47000 at 72 x 40: 2.17e9 doubles of qtens (17.3 GB), generated on the device.  Element 0, the element
    that contains double index 2^31, its two neighbours and the last element against both references; isfinite on the
    whole array.  Needs 21 GiB of device memory."""
    import torch
    need = 21
    free = torch.cuda.mem_get_info()[0]
    if free < need * 2 ** 30:
        pytest.skip(f"memory shortfall: this case needs {need} GiB of device memory, torch.cuda.mem_get_info reports "
                    f"{free / 2 ** 30:.1f} GiB free")
    nelemd, nlev, qsize = 47000, 72, 40
    per = 16 * nlev * qsize
    mid = 2 ** 31 // per
    assert nelemd * per > 2 ** 31 and 0 < mid - 1 and mid + 1 < nelemd - 1
    g = torch.Generator(device="cuda:0").manual_seed(11)
    q = torch.rand((nelemd, qsize, nlev, 4, 4), dtype=torch.float64, device="cuda:0", generator=g)
    q.sub_(0.5)
    el = torch.rand((nelemd, 144), dtype=torch.float64, device="cuda:0", generator=g) - 0.5
    dv = torch.rand((4, 4), dtype=torch.float64, device="cuda:0", generator=g) - 0.5
    picks = (0, mid - 1, mid, mid + 1, nelemd - 1)
    q0 = {ie: q[ie].clone() for ie in picks}
    K.set_variant(variant)
    K.biharmonic_wk_scalar(el, q, dv)
    torch.cuda.synchronize()
    ok = True
    for c0 in range(0, nelemd, 4700):
        ok = ok and bool(torch.isfinite(q[c0:c0 + 4700]).all())
    assert ok
    for ie, qin in q0.items():
        inp = {"dvv": to_host(dv), "elem": to_host(el[ie:ie + 1]), "qtens": to_host(qin[None])}
        out = to_host(q[ie:ie + 1])
        if variant == 0:
            assert_bitwise(out, B.biharmonic(inp), f"element {ie}")
        hi, S = B.biharmonic_hi(inp)
        within_bound(B, out, hi, S, f"17 GB element {ie} variant={variant}", (("exact", "fast")[variant], "large"))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["exact", "fast"])
def test_c3_placement_guard_bands_and_inputs_untouched(K, B, variant):
    """dvv at 8 modulo 32, qtens and elem at 32 modulo 64 (the least the header allows): bit-identical to the aligned
    run.  4 KiB of NaN-payload sentinel on both sides of qtens stay intact; elem and dvv are unchanged."""
    import torch
    for shape in [(3, 9, 5), (2, 31, 33), (7, 1, 1)]:
        inp = B.random_inputs(*shape, seed=sum(shape))
        aligned = run_hip(K, inp, variant)
        band, off = 512, 4                                            # doubles: 4 KiB; 32 bytes
        nq = inp["qtens"].size
        qbuf = torch.full((band + off + nq + band,), SENTINEL, dtype=torch.int64, device="cuda:0").view(torch.float64)
        q = qbuf[band + off:band + off + nq].view(to_dev(inp["qtens"]).shape)
        q.copy_(to_dev(inp["qtens"]))
        ebuf = torch.zeros(inp["elem"].size + 8, dtype=torch.float64, device="cuda:0")
        el = ebuf[off:off + inp["elem"].size].view(shape[0], 144)
        el.copy_(to_dev(inp["elem"]))
        dbuf = torch.zeros(24, dtype=torch.float64, device="cuda:0")
        dv = dbuf[1:17].view(4, 4)
        dv.copy_(to_dev(inp["dvv"]))
        assert q.data_ptr() % 64 == 32 and el.data_ptr() % 64 == 32 and dv.data_ptr() % 32 == 8
        el0, dv0 = el.clone(), dv.clone()
        K.set_variant(variant)
        K.biharmonic_wk_scalar(el, q, dv)
        torch.cuda.synchronize()
        assert_bitwise(to_host(q), aligned, f"placement {shape}")
        raw = qbuf.view(torch.int64)
        assert bool((raw[:band + off] == SENTINEL).all()) and bool((raw[band + off + nq:] == SENTINEL).all()), shape
        assert torch.equal(el.view(torch.int64), el0.view(torch.int64)) and torch.equal(dv.view(torch.int64), dv0.view(torch.int64))


@pytest.mark.gpu
def test_report_ratios():
    """(runs last in this module) the worst |out - hi| / (gamma(c) S) per variant and regime, for the record"""
    from oracle.bwk import PATH_ROUNDINGS
    for (variant, regime), (ratio, what) in sorted(WORST.items()):
        print(f"BWK {variant:6s} {regime:14s} worst |out - hi| / (gamma({PATH_ROUNDINGS}) S) = {ratio:.4f}   ({what})")
    assert all(r <= 1.0 for r, _ in WORST.values())
