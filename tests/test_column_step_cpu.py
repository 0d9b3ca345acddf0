"""CPU tests of the fused column step (include/mpdata_hip.h 3q): the numpy model of tests/column_step_model.py against the
chain of the four plan models of the single sections for every non-empty subset of the stages, the plan model's rules, and
the interface (header, ctypes, Fortran, Python names, the argument checks that need no device, the compiler's resource
report).  No test here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cell_add_model as CM
import column_step_model as QM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from oracle import plan_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpdata_plan_column_step_device", "mpdata_plan_column_step", "mpdata_plan_column_step_f32", "mpdata_column_step_device",
         "mpdata_column_step_f32_device")
DTYPES = [np.float64, np.float32]
SHAPE, T = (5, 4, 9), 2


class Chain(UM.PlanModelSubside, SM.PlanModelSediment, VM.PlanModelVsolve, CM.PlanModelCellAdd):
    """the four single calls on one plan model"""


def _models(oracle, dtype, seed=100):
    inp = QM.make_plan_inputs(oracle, SHAPE, T, dtype, seed)
    a, b = QM.PlanModelColumnStep(oracle, *SHAPE, T, dtype), Chain(oracle, *SHAPE, T, dtype)
    for m in (a, b):
        assert m.upload({k: np.array(v, order="F") for k, v in inp.items()}) is None
    return a, b, inp


# ---- the model against the sequence of the single calls
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("stages", QM.SUBSETS, ids=["+".join(s) for s in QM.SUBSETS])
def test_model_is_the_chain_of_the_single_calls(oracle, stages, dtype):
    """on a block and a tracer range: the interior columns bit for bit, the halos those of the input (the chain's subside
    changes them; the fused call does not), psfc the sediment call's; c = 0.1 is no fp32 number"""
    a, b, inp = _models(oracle, dtype)
    ncrms, nx, nz = SHAPE
    sl0, n, first, ntr = 1, 3, 0, 2
    c = 0.1 if dtype == np.float32 else 0.75
    kw = QM.make_args(n, nx, nz, ntr, dtype, 40, stages)
    before = np.array(a.a["f"], order="F")
    if "source" in stages:
        frac = CM.clipped_fraction(before[sl0:sl0 + n], kw["s"], c)
        assert 0.2 <= frac <= 0.8, frac
    ps = a.column_step(c=c, mode=QM.CLIP, psfc="sediment" in stages, sl0=sl0, n=n, first=first, ntr=ntr, **kw)
    assert not isinstance(ps, int), ps
    blk = dict(sl0=sl0, n=n, first=first, ntr=ntr)
    want_ps = None
    if "source" in stages:
        assert not isinstance(b.cell_add(kw["s"], c, CM.CLIP, **blk), int)
    if "subside" in stages:
        assert not isinstance(b.subside(kw["cb"], kw["cc"], **blk), int)
    if "sediment" in stages:
        want_ps, _ = b.sediment(kw["wp"], **blk)
    if "vsolve" in stages:
        assert b.vsolve(kw["lo"], kw["di"], kw["up"], **blk) is None
    got, want = a.a["f"], b.a["f"]
    assert np.array_equal(QM.bits(got[:, 3:nx + 3]), QM.bits(want[:, 3:nx + 3]))
    assert np.array_equal(QM.bits(got[:, :3]), QM.bits(before[:, :3])) and np.array_equal(QM.bits(got[:, nx + 3:]), QM.bits(before[:, nx + 3:]))
    assert not np.array_equal(got[sl0:sl0 + n, 3:nx + 3], before[sl0:sl0 + n, 3:nx + 3])
    outside = np.ones(ncrms, bool)
    outside[sl0:sl0 + n] = False
    assert np.array_equal(QM.bits(got[outside]), QM.bits(before[outside]))
    if "subside" in stages:
        assert not np.array_equal(want[sl0:sl0 + n, :3], before[sl0:sl0 + n, :3])     # (the difference from the sequence is real)
    if "sediment" in stages:
        assert np.array_equal(QM.bits(ps), QM.bits(want_ps))
    else:
        assert ps is None
    for k in ("u", "w", "rho", "rhow", "adz", "flux"):
        assert np.array_equal(QM.bits(a.a[k]), QM.bits(b.a[k])), k
    # a run and a read-back behind the call see the same field, whatever the halos held (PERIODIC: every read wraps)
    for m in (a, b):
        assert m.set_boundary(PM.PERIODIC) is None and m.run() is None
    ea, eb = a.export_device(), b.export_device()
    for k in ea:
        assert np.array_equal(QM.bits(ea[k]), QM.bits(eb[k])), k


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_psfc_is_of_the_field_that_enters_the_stage_and_the_order_matters(dtype):
    n, nx, nz = 2, 3, 7
    rng = np.random.default_rng(3)
    f = np.asfortranarray(rng.uniform(-0.5, 0.5, (n, nx + 6, nz - 1)).astype(dtype))
    rho, adz = (np.asfortranarray(rng.uniform(0.5, 1.0, (n, nz - 1)).astype(dtype)) for _ in range(2))
    kw = QM.make_args(n, nx, nz, None, dtype, 9)
    new, ps = QM.column_step(f, rho, adz, c=0.75, mode=QM.ADD, **kw)
    g, _ = CM.cell_add(f, kw["s"], 0.75, CM.ADD)
    g, _ = UM.subside(g, kw["cb"], kw["cc"])
    assert np.array_equal(QM.bits(ps), QM.bits(kw["wp"][:, :, 0] * g[:, 3:nx + 3, 0]))
    assert not np.array_equal(ps, kw["wp"][:, :, 0] * new[:, 3:nx + 3, 0])
    # sediment before subside is another result
    h, _ = CM.cell_add(f, kw["s"], 0.75, CM.ADD)
    h, _, _ = SM.sediment(h, rho, adz, kw["wp"])
    h, _ = UM.subside(h, kw["cb"], kw["cc"])
    h = VM.vsolve(h, kw["lo"], kw["di"], kw["up"])
    assert not np.array_equal(h[:, 3:nx + 3], new[:, 3:nx + 3])


def test_plan_model_errors_in_order_and_change_nothing(oracle):
    a, _, inp = _models(oracle, np.float64)
    ncrms, nx, nz = SHAPE
    kw = QM.make_args(ncrms, nx, nz, T, np.float64, 6)
    fresh = QM.PlanModelColumnStep(oracle, *SHAPE, T, np.float64)
    assert fresh.column_step(**kw) == PM.ESTATE                               # never filled
    keep = {k: np.array(v) for k, v in a.a.items()}
    for sl0, n in ((0, 0), (0, -1), (-1, 2), (0, 6), (5, 1), (3, 3)):
        assert a.column_step(sl0=sl0, n=n, **kw) == PM.EINVAL, (sl0, n)
    assert a.column_step(first=1, ntr=2, **kw) == PM.EINVAL and a.column_step(first=0, ntr=0, **kw) == PM.EINVAL
    assert a.column_step() == PM.EINVAL                                       # no stage
    assert a.column_step(cb=kw["cb"]) == PM.EINVAL and a.column_step(cc=kw["cc"]) == PM.EINVAL
    assert a.column_step(lo=kw["lo"]) == PM.EINVAL and a.column_step(lo=kw["lo"], up=kw["up"]) == PM.EINVAL
    assert a.column_step(s=kw["s"], psfc=True) == PM.EINVAL                   # psfc without wp
    assert a.column_step(s=kw["s"], mode=2) == PM.EINVAL
    assert not isinstance(a.column_step(wp=kw["wp"], mode=7), int)            # the mode is ignored without s
    a.a = {k: np.array(v) for k, v in keep.items()}
    assert a.column_step(eb=4, **kw) == PM.ESTATE                             # a host form of the other precision
    assert a.column_step(eb=4) == PM.EINVAL and a.column_step(s=kw["s"], mode=2, eb=4) == PM.EINVAL   # the NULLs and the mode first
    a.windowed = True
    assert a.column_step(**kw) == PM.EUNSUPPORTED and a.column_step() == PM.EINVAL and a.column_step(eb=4, **kw) == PM.EUNSUPPORTED
    a.windowed = False
    a.multi = True
    assert a.column_step(**kw) == PM.EUNSUPPORTED and a.column_step(sl0=0, n=0, **kw) == PM.EINVAL
    assert a.column_step() == PM.EUNSUPPORTED                                 # the handle comes before the NULLs
    a.multi = False
    for k, v in keep.items():
        assert np.array_equal(QM.bits(a.a[k]), QM.bits(v)), k


# ---- the interface (files parsed: no device)
def test_python_names(mpdata):
    assert callable(mpdata.column_step_device) and callable(mpdata.Plan.column_step_device) and callable(mpdata.Plan.column_step)
    for nm in ("column_step_device", "column_step_shapes"):
        assert nm in mpdata.__all__, nm
    sh = mpdata.column_step_shapes(5, 3, 8)
    assert sh["s"] == sh["wp"] == (7, 3, 5) and sh["psfc"] == (3, 5)
    assert all(sh[k] == (7, 5) for k in ("cb", "cc", "lo", "di", "up"))
    sh = mpdata.column_step_shapes(5, 3, 8, 2)
    assert sh["s"] == sh["wp"] == (2, 7, 3, 5) and sh["psfc"] == (2, 3, 5) and sh["cb"] == (7, 5)


def _c_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"header: {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_section():
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    assert "---- 3q." in hdr
    assert hdr.index("---- 3p.") < hdr.index("---- 3q.") < hdr.index("---- 4.")
    sec = hdr.split("---- 3q.")[1].split("---- 4.")[0]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", sec), n
    assert "FIXED ORDER" in sec and re.search(r"1\. source.*2\. subside.*3\. sediment.*4\. vsolve", sec, re.S)
    assert "windowed" in sec.lower() and "MPDATA_EUNSUPPORTED" in sec and "mpdata_plan_shard_plan" in sec
    assert "differs from that sequence in two places" in sec and "halo slots" in sec and "horizontal sums" in sec
    assert "neither reads nor writes halo columns" in sec and "NOT offered" in sec
    assert "ENTERS this stage" in sec and "rounded ONCE" in sec and "BIT FOR BIT" in sec


def test_library_exports_and_ctypes_agree_with_the_header(mpdata):
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    L = mpdata.lib()
    ckind = {ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_void_p: "*", ctypes.c_double: "double", ctypes.c_float: "float"}
    for n in NAMES:
        params = _c_params(hdr, n)
        fn = getattr(L, n)                                   # the library exports it
        assert fn.restype is ctypes.c_int and fn.argtypes is not None and len(fn.argtypes) == len(params), n
        for a, p in zip(fn.argtypes, params):
            k = ckind[a]
            assert ("*" in p) if k == "*" else (p.startswith(k + " ") and "*" not in p), (n, p, a)
    assert _c_params(hdr, "mpdata_plan_column_step_device")[4] == "double c"
    assert _c_params(hdr, "mpdata_plan_column_step_f32")[4] == "float c" and _c_params(hdr, "mpdata_column_step_f32_device")[10] == "float c"
    assert len(_c_params(hdr, "mpdata_plan_column_step_device")) == 15 and len(_c_params(hdr, "mpdata_column_step_device")) == 20


def test_fortran_interface_agrees_with_the_header():
    """the one interface, bound by the literal name, public, in the interface block of the bindings with a real by value,
    the dummy arguments in the header's order, each of the header's kind and passed by value"""
    hdr = open(os.path.join(ROOT, "include", "mpdata_hip.h")).read()
    f90 = open(os.path.join(ROOT, "codesign-kernels_amd", "fortran", "mpdata_hip_mod.F90")).read()
    m = re.search(r"integer\(c_int\) function mpdata_plan_column_step_device_c\(([^)]*)\)\s*&?\s*bind\(C, name=\"mpdata_plan_column_step_device\"\)"
                  r"(.*?)end function", f90, re.S)
    assert m
    fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    params = _c_params(hdr, "mpdata_plan_column_step_device")
    cargs = [re.split(r"[\s*]+", p)[-1] for p in params]
    assert fargs == cargs, (fargs, cargs)
    decl = {}
    for line in m.group(2).splitlines():
        d = re.match(r"\s*(type\(c_ptr\)|integer\(c_int64_t\)|integer\(c_int\)|real\(c_double\))\s*,\s*value\s*::\s*(.*)", line)
        if d:
            for a in d.group(2).split(","):
                decl[a.strip()] = d.group(1)
    assert len(decl) == len(params) == 15
    for p, a in zip(params, cargs):
        want = ("type(c_ptr)" if "*" in p else "integer(c_int64_t)" if p.startswith("int64_t ") else
                "real(c_double)" if p.startswith("double ") else "integer(c_int)")
        assert decl.get(a) == want, (a, p, decl.get(a))
    assert decl["c"] == "real(c_double)"
    assert "c_double" in re.search(r"import ::(.*)", m.group(2)).group(1)
    assert re.search(r"public ::.*\bmpdata_plan_column_step_device_c\b", f90)
    # the second interface block: the one that holds 3p's binding
    blocks = re.findall(r"\n  interface\n(.*?)\n  end interface", f90, re.S)
    assert len(blocks) == 2 and "mpdata_plan_column_step_device_c" not in blocks[0]
    assert "mpdata_plan_column_step_device_c" in blocks[1] and "mpdata_plan_cell_add_device_c" in blocks[1]
    # (its make rule and its .gitignore entry: tests/test_fortran_plan_calls.py, for every program at once)
    assert os.path.exists(os.path.join(ROOT, "tests", "fortran", "column_step_calls.F90"))


def test_argument_errors_without_device(mpdata):
    L = mpdata.lib()
    E = mpdata.EINVAL
    err = L.mpdata_last_error
    one = ctypes.c_void_p(8)   # never dereferenced: the checks come before anything looks at the arrays
    for fn in (L.mpdata_column_step_device, L.mpdata_column_step_f32_device):
        def call(sizes=(4, 5, 6, 1), blk=(0, 4), f=one, rho=one, adz=one, s=one, mode=0, cb=one, cc=one, wp=one, psfc=None, lo=one, di=one,
                 up=one):
            return fn(*sizes, *blk, f, rho, adz, s, 1.0, mode, cb, cc, wp, psfc, lo, di, up, None)
        assert call(sizes=(4, 0, 6, 1)) == E and call(sizes=(0, 5, 6, 1)) == E and call(sizes=(4, 5, 6, 0)) == E
        assert call(sizes=(4, 5, 1, 1)) == E and b"nz=1" in err()
        for blk in ((0, 0), (-1, 2), (0, 5), (4, 1), (2, 3)):
            assert call(blk=blk) == E and b"outside" in err(), blk
        assert call(f=None) == E and b"null f" in err()
        none = dict(s=None, cb=None, cc=None, wp=None, lo=None, di=None, up=None)
        assert call(**none) == E and b"no stage" in err()
        assert call(f=None, **none) == E and b"null f" in err()                                  # f comes first
        assert call(cc=None) == E and b"cb without cc" in err() and call(cb=None) == E and b"cc without cb" in err()
        assert call(di=None) == E and b"null di" in err() and call(lo=None, up=None) == E and b"null lo" in err()
        assert call(wp=None, psfc=one) == E and b"psfc without wp" in err()
        for mode in (2, -1, 7):
            assert call(mode=mode) == E and b"unknown mode" in err()
        assert call(mode=7, cc=None) == E and b"cb without cc" in err()                          # the NULLs before the mode
        assert call(rho=None) == E and b"null rho" in err() and call(adz=None) == E and b"null adz" in err()
        assert call(rho=None, mode=7) == E and b"unknown mode" in err()                          # ... and rho, adz behind it
        assert call(sizes=(4, 5, 1, 1), f=None, **none) == E and b"nz=1" in err()
    P = L.mpdata_plan_column_step_device
    assert P(None, 0, 1, one, 1.0, 0, one, one, one, None, one, one, one, 0, 1) == E and b"null plan" in err()
    assert L.mpdata_plan_column_step(None, 0, 1, one, 1.0, 0, one, one, one, None, one, one, one) == E
    assert L.mpdata_plan_column_step_f32(None, 0, 1, one, 1.0, 0, one, one, one, None, one, one, one) == E
    for n, sl0 in ((0, 0), (-2, 0), (1, -1)):   # (checked before the plan is looked at)
        assert P(one, sl0, n, one, 1.0, 0, one, one, one, None, one, one, one, 0, 1) == E
    assert P(one, 0, 0, None, 1.0, 9, None, None, None, None, None, None, None, 0, 1) == E
    assert b"no stage" not in err() and b"unknown mode" not in err()                             # the range came first


def test_new_kernels_do_not_spill_and_fit_the_lds_budget():
    """the resource-usage report the build writes next to the object of mpdata_column_step.hip: no scratch memory, no vector
    and no scalar register spilled in any kernel; the LDS of the plan-layout kernel is dynamic, its budget a constant of
    the file: 40 KiB at most, four workgroups per CU"""
    csrc = os.path.join(ROOT, "codesign-kernels_amd", "csrc")
    rep = os.path.join(csrc, "mpdata_column_step.usage.txt")
    assert os.path.exists(rep), f"{rep}: the build writes it"
    txt = open(rep).read()
    # one kernel per set of stages, layout and precision; the small kernel of 1 / (rho * adz) in both
    assert len(re.findall(r"Function Name: \S*wm_column_step_kernel", txt)) == 30
    assert len(re.findall(r"Function Name: \S*ref_column_step_kernel", txt)) == 30
    assert len(re.findall(r"Function Name: \S*wm_ir_kernel", txt)) == 2
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == 62 and set(scratch) == {0}
    assert {int(x) for x in re.findall(r"VGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"SGPRs Spill: (\d+)", txt)} == {0}
    assert {int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", txt)} == {0}      # (static: none; the dynamic size below)
    # four workgroups of 256 per CU need 128 vector registers at most in the plan-layout kernels
    for blk in re.split(r"Function Name: ", txt)[1:]:
        if "wm_column_step_kernel" in blk.split()[0]:
            assert int(re.search(r" VGPRs: (\d+)", blk).group(1)) <= 128
    src = open(os.path.join(csrc, "mpdata_column_step.hip")).read()
    walk = open(os.path.join(csrc, "mpdata_wm_walk.h")).read()
    m = re.search(r"constexpr int LDS_ELEMS = (\d+);", walk)                               # (the one statement of the limit)
    assert m and int(m.group(1)) * 8 <= 40 * 1024
    assert "col_groups_batched(j, b.sel, wg, LDS_ELEMS," in src and "g->lds_e <= budget" in walk     # the launch refuses more
    assert "asm" not in re.sub(r"//.*", "", src)                                             # plain C++
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"mpdata_column_step\$\(O\):.*\n\t\$\(call CC_USAGE,-ffp-contract=off,", mk)
