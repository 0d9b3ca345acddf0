"""The Fortran face of the plan API, executed: tests/fortran/plan_calls.F90 drives a resident plan through the interfaces of
codesign-kernels_amd/fortran/mpdata_hip_mod.F90 alone (include/mpdata_hip.h sections 3 - 3l), and this module replays the
program's script on ONE numpy model that joins the two model chains of the suite -- tests/diffuse_model.py PlanModelDiffuse and
tests/column_path_model.py PlanModelPath (which holds level_add and scale_uw), with level_stats_model.level_stats and
courant_model.courant on the arrays it holds.

GPU tests: one run of the program per case.  The test writes the program's inputs, runs it, parses its dump and compares every
record -- every array and the return code of every call -- with the replay, bit for bit, in the program's order.  ncycle and su
are formed in numpy from the MODEL's cinst and must equal the program's.  -0.0 is canonicalised (AM.canon) on both sides only
for f read back after a level_add CLIP, as tests/test_plan_level_add.py does.  The inputs are built so that in every step the
plan holds an instance with ncycle = 1 and one with ncycle >= 2, none above 3 -- asserted on the model before the program
runs, over the plan, over the block where it has two instances, and over the steps where it has one.
A one-tracer plan has no tracers [0, T-1): the program leaves that diffuse call out there.

The EXACT variant only: the bindings do not depend on the variant, and what the block calls do on a FAST plan is covered by the
tests of each call (tests/test_plan_level_add.py, test_plan_scale_uw.py, test_plan_diffuse.py, ...).

CPU tests: the module's text against the header -- every bind(C) interface in count, order AND kind of its dummy arguments, the
symbol every per-precision macro names, what is public, the identifiers of INTEGRATION.md's Fortran snippets -- and the two
programs build() leaves behind."""
import functools
import glob
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import column_path_model as CP
import courant_model as CM
import diffuse_model as DM
import fortran_records as FR
import level_add_model as AM
import level_stats_model as LM
import scale_uw_model as SM
from oracle import plan_model as PM
from test_periodic_api import wrap
from util import assert_bitwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "codesign-kernels_amd", "fortran")
MODULE = os.path.join(FDIR, "mpdata_hip_mod.F90")
HEADER = os.path.join(ROOT, "include", "mpdata_hip.h")
TDIR = os.path.join(ROOT, "tests", "fortran")
EXE = {np.float64: "plan_calls", np.float32: "plan_calls_sp"}
# every test program, by its source; the suffix of the executable per precision
PROGRAMS = sorted(os.path.basename(p)[:-len(".F90")] for p in glob.glob(os.path.join(TDIR, "*_calls.F90")))
SUFFIX = {np.float64: "", np.float32: "_sp"}
COMMON = "calls_common"          # tests/fortran/calls_common.F90: what the programs share
SENTINEL, FACTOR, S = -777.0, 0.75, 3


# ------------------------------------------------------------------------------------------------ the cases
# name -> shape, tracers, dtype, the block (sl0, n) of the block calls, the block of the instance calls (inside the plan where
# the plan has room for one), the tracers (first, count) of the CLIP, the switches.  ncrms, nx, nzm, T, sl0, n differ from one
# another wherever the case leaves the choice, so that two integers swapped on the way land on other data.
def _c(shape, T, dt, block, iblock, clip, odd=False, tall=False, seed=100):
    return dict(shape=shape, T=T, dt=dt, block=block, iblock=iblock, clip=clip, odd=odd, tall=tall, seed=seed)


CASES = {
    "f64-block": _c((7, 5, 10), 3, np.float64, (2, 3), (1, 4), (1, 2)),
    "f64-whole": _c((7, 5, 10), 3, np.float64, (0, 7), (1, 4), (1, 2)),
    "f32-even": _c((6, 5, 10), 3, np.float32, (1, 3), (3, 2), (1, 2)),                    # both blocks split instance pairs
    "f32-odd": _c((7, 5, 10), 2, np.float32, (6, 1), (1, 4), (1, 1), odd=True),           # the instance beside the phantom half
    "f64-nz72": _c((3, 4, 72), 1, np.float64, (1, 2), (1, 1), (0, 1)),                    # an instance spans two waves
    "f64-windowed": _c((2, 4, 250), 1, np.float64, (0, 2), (1, 1), (0, 1), tall=True),    # (two instances: no inner block)
}


def make_case(oracle, name):
    """the records of the program's input file, in its order, as a dict"""
    c = CASES[name]
    shape, T, dt, seed = c["shape"], c["T"], c["dt"], c["seed"]
    ncrms, nx, nz = shape
    (sl0, n), (t1, tn) = c["block"], c["clip"]
    inp = DM.make_plan_inputs(oracle, shape, T, dt, seed)
    r = {k: np.asfortranarray(inp[k]) for k in PM.NAMES}
    r["f"] = np.asfortranarray(r["f"].reshape(ncrms, nx + 6, nz - 1, T, order="F"))
    r["flux"] = np.asfortranarray(r["flux"].reshape(ncrms, nz, T, order="F"))
    small = dt(2.0 ** -5)              # raw u, w in [-0.5, 0.5), rho, adz >= 0.5: an outflow Courant number below 3/16
    r["u"], r["w"] = np.asfortranarray(r["u"] * small), np.asfortranarray(r["w"] * small)
    us, ws = [], []
    for s in range(S):
        o = oracle.make_inputs(*shape, seed=seed + 10 * (s + 1), dist=oracle.DIST_RAW_SIGNED, dtype=dt)
        us.append(o["u"] * small)
        ws.append(o["w"] * small)
    c0 = [CM.courant(us[s], ws[s], r["rho"], r["adz"])[1] for s in range(S)]
    cmax = max(float(x.max()) for x in c0)
    # instance sl of step s is left alone (ncycle = 1) where sl + s is odd; the others are scaled to 1.5 cmax (ncycle = 2),
    # every fourth to 2.5 cmax (ncycle = 3): half a unit away from where the ceiling jumps
    for s in range(S):
        for sl in range(ncrms):
            if (sl + s) % 2 == 0:
                g = dt((2.5 if sl % 4 == 0 else 1.5) * cmax / float(c0[s][sl]))
                us[s][sl] *= g
                ws[s][sl] *= g
    r["us"], r["ws"] = np.asfortranarray(np.stack(us, -1)), np.asfortranarray(np.stack(ws, -1))
    co = [DM.make_coeffs(n, nx, nz, dt, seed + 1 + s) for s in range(S)]
    for k in ("tkh", "cx", "cz", "sb", "st"):
        r[k] = np.asfortranarray(np.stack([x[k] for x in co], -1))
    r["dclip"] = np.asfortranarray(np.stack([AM.make_d(shape, tn, dt, seed + 20 + s, n).reshape(n, nz - 1, tn, order="F")
                                             for s in range(S)], -1))
    r["dadd"] = np.asfortranarray(np.stack([AM.make_d(shape, T, dt, seed + 40 + s, n).reshape(n, nz - 1, T, order="F")
                                            for s in range(S)], -1))
    r["ad"] = np.asfortranarray(AM.make_d(shape, T, dt, seed + 60).reshape(ncrms, nz - 1, T, order="F"))
    r["asu"], r["asw"] = SM.make_s(shape, dt, seed + 70), SM.make_s(shape, dt, seed + 1070)
    assert not np.array_equal(r["asu"], r["asw"])
    params = np.array([ncrms, nx, nz, T, sl0, n, *c["iblock"], S, t1, tn, int(c["odd"]), int(c["tall"])], np.int64)
    out = {"params": params, "cmax": np.array([cmax], dt)}
    for k in ("f", "u", "w", "rho", "rhow", "adz", "flux", "us", "ws", "tkh", "cx", "cz", "sb", "st", "dclip", "dadd", "ad", "asu", "asw"):
        assert r[k].dtype == np.dtype(dt), k
        out[k] = r[k]
    return out


class Model(DM.PlanModelDiffuse, CP.PlanModelPath):
    """one plan model with every in-place call: 3l beside 3i, 3j and 3k (the two chains of the suite, joined)"""


def ncycle_of(cinst, cmax):
    """the program's three lines: ncycle = max(1, ceiling(cinst / cmax)), su = 1 / ncycle, in the plan's precision"""
    dt = cinst.dtype.type
    q = cinst / dt(cmax)
    assert q.dtype == cinst.dtype
    ncycle = np.maximum(1, np.ceil(q)).astype(np.int32)
    su = dt(1) / ncycle.astype(cinst.dtype)
    assert su.dtype == cinst.dtype
    return ncycle, su


def replay(oracle, mpdata, name, inputs):
    """the program's script on the model -> ([(record name, array)] in the program's order, the ncycle of every step over the
    whole plan)"""
    c = CASES[name]
    ncrms, nx, nz = c["shape"]
    T, dt = c["T"], c["dt"]
    (sl0, n), (bsl0, bn), (t1, tn) = c["block"], c["iblock"], c["clip"]
    cmax = inputs["cmax"][0]
    b = slice(sl0, sl0 + n)
    out, plan_ncycle = [], []

    def rc(what, code=0):
        out.append(("rc:" + what, np.array([0 if code is None else code], np.int32)))

    def rec(what, a):
        out.append((what, np.asfortranarray(a)))

    def sentinel(*shape):
        return np.full(shape, SENTINEL, dt, order="F")

    def result(r, *shape):
        """a model call's (return code, output): an MPDATA_E* code leaves the output as the program set it"""
        return (r, sentinel(*shape)) if isinstance(r, int) else (0, r)

    m = Model(oracle, ncrms, nx, nz, T, dt)
    m.windowed = c["tall"]
    rc("set_variant")
    if c["odd"]:
        rc("set_f32_odd")
    if c["tall"]:
        rc("set_tall")
    rc("create")
    rc("set_boundary", m.set_boundary(PM.PERIODIC))
    rc("upload", m.upload({k: np.array(inputs[k], order="F") for k in PM.NAMES}))
    rc("boundary", PM.PERIODIC)
    W = mpdata.level_window(nz, 0)[0] if c["tall"] else 1
    assert (W > 1) == c["tall"]
    rc("level_windows", W)
    for s in range(S):
        rc("import_uw", m.import_device({"u": np.array(inputs["us"][..., s], order="F"), "w": np.array(inputs["ws"][..., s], order="F")}, 0, T))
        clev, cinst = CM.courant(m.a["u"][b], m.a["w"][b], m.a["rho"][b], m.a["adz"][b])
        plan_ncycle.append(ncycle_of(CM.courant(m.a["u"], m.a["w"], m.a["rho"], m.a["adz"])[1], cmax)[0])
        if s % 2 == 0:
            rc("courant_host")
        else:
            rc("courant_dev")
            rc("sync")
        rec("clev", clev)
        rec("cinst", cinst)
        ncycle, su = ncycle_of(cinst, cmax)
        rec("ncycle", ncycle)
        rec("su", su)
        if s == 0:
            rc("scale_host", m.scale_uw(su, su, sl0, n))
        elif s == 1:
            rc("scale_dev", m.scale_uw(su, su, sl0, n))
        else:
            rc("scale_host_u", m.scale_uw(su, None, sl0, n))
            rc("courant_mid")
            rec("cinst_mid", CM.courant(m.a["u"][b], m.a["w"][b], m.a["rho"][b], m.a["adz"][b])[1])
            rc("scale_dev_w", m.scale_uw(None, su, sl0, n))
        for _ in range(int(ncycle.max())):
            assert m.run() is None
        rc("runs", int(ncycle.max()))
        rc("run")
        rc("sync")
        co = {k: np.asfortranarray(inputs[k][..., s]) for k in ("tkh", "cx", "cz", "sb", "st")}
        if s == 1:
            code, z = result(m.diffuse(**co, sl0=sl0, n=n, first=0, ntr=T, eb=np.dtype(dt).itemsize), n, nz, T)
            rc("diffuse_host", code)
            rec("zflux_h", z)
        else:
            if T > 1:
                code, z = result(m.diffuse(**co, sl0=sl0, n=n, first=0, ntr=T - 1), n, nz, T - 1)
                rc("diffuse_dev_a", code)
                rc("sync")
                rec("zflux_a", z)
            code, z = result(m.diffuse(**dict(co, sb=None), sl0=sl0, n=n, first=T - 1, ntr=1), n, nz, 1)
            rc("diffuse_dev_b", code)
            rc("sync")
            rec("zflux_b", z)
        assert m.finite()
        st = LM.level_stats(m.a["f"][b])
        rc("stats_dev")
        rc("sync")
        rec("sum_d", st[0])
        rec("min_d", st[1])
        rc("stats_host")
        for k, a in zip(("sum_h", "min_h", "max_h"), st):
            rec(k, a)
        rc("add_clip_dev", m.level_add(np.asfortranarray(inputs["dclip"][..., s]), sl0, n, AM.CLIP, t1))
        rc("sync")
        rc("add_host", m.level_add(np.asfortranarray(inputs["dadd"][..., s]), sl0, n, AM.ADD, 0))
        assert m.column_path(sl0, n) is None
        path, mass = m.paths(sl0, n)
        rc("path_dev")
        rc("sync")
        rec("path_d", path)
        rec("mass_d", sentinel(n, T) if s == 0 else mass)
        rc("path_host")
        rec("path_h", path)
        rec("mass_h", mass)
        blk = m.export_block(bsl0, bn)
        rc("export_block")
        rc("sync")
        rec("f_eb", blk["f"])
        rec("flux_eb", blk["flux"])
        rc("download_blk")
        rec("f_db", blk["f"])
        rec("flux_db", blk["flux"])
        fb = blk["f"] * dt(FACTOR)
        assert fb.dtype == np.dtype(dt)
        rc("import_block", m.import_block(bsl0, bn, {"f": fb}, 0, T))
        rc("sync")
    whole = m.export_device()
    rc("export")
    rc("sync")
    rec("f_e", whole["f"])
    rec("flux_e", whole["flux"])
    rc("download")
    rec("f_d", whole["f"])
    rec("flux_d", whole["flux"])
    rc("last_ms", 0 if m.last_kernel_ms() is True else m.last_kernel_ms())
    rc("ms_positive", 1)
    rc("destroy")
    # the array forms, on the arrays the plan was filled with
    F, U, Wv = (np.array(inputs[k], order="F") for k in ("f", "u", "w"))
    rho, adz = inputs["rho"], inputs["adz"]
    st = LM.level_stats(F)
    rc("a_stats")
    F = AM.level_add(F, inputs["ad"], clip=True)
    rc("a_add")
    co = {k: np.asfortranarray(inputs[k][..., 0]) for k in ("tkh", "cx", "cz", "sb", "st")}
    F[b], zf = DM.diffuse(F[b], rho[b], adz[b], **co)
    rc("a_diffuse")
    path, mass = CP.column_path(F, rho, adz)
    rc("a_path")
    clev, cinst = CM.courant(U, Wv, rho, adz)
    rc("a_courant")
    U, Wv = SM.scale_uw(U, Wv, inputs["asu"], inputs["asw"])
    rc("a_scale")
    wrap(f=F, u=U, w=Wv)
    rc("a_halo")
    rc("device_sync")
    for k, a in (("a_sum", st[0]), ("a_min", st[1]), ("a_max", st[2]), ("a_zflux", zf), ("a_path", path), ("a_mass", mass),
                 ("a_clev", clev), ("a_cinst", cinst), ("a_f", F), ("a_u", U), ("a_w", Wv)):
        rec(k, a)
    return out, plan_ncycle


CANON = ("f_eb", "f_db", "f_e", "f_d", "a_f")      # f read back behind a level_add CLIP


def compare(got, want, what):
    for i, ((gn, ga), (wn, wa)) in enumerate(zip(got, want)):
        assert gn == wn, f"{what}: record {i} of the dump is {gn!r}, the script's is {wn!r}"
        assert ga.dtype == wa.dtype and ga.shape == wa.shape, f"{what}: record {i} {gn}: {ga.dtype}{ga.shape}, expected {wa.dtype}{wa.shape}"
        if gn.startswith("rc:") or ga.dtype.kind == "i":
            assert np.array_equal(ga, wa), f"{what}: record {i} {gn}: {ga.tolist()}, expected {wa.tolist()}"
        elif gn in CANON:
            assert_bitwise(AM.canon(ga), AM.canon(wa), f"{what}: record {i} {gn}")
        else:
            assert_bitwise(ga, wa, f"{what}: record {i} {gn}")
    assert len(got) == len(want), f"{what}: {len(got)} records in the dump, {len(want)} in the script"


def check_subcycling(name, want, plan_ncycle):
    """the condition on the inputs: every step holds an instance with ncycle = 1 and one with ncycle >= 2, none above 3"""
    n = CASES[name]["block"][1]
    block = [a for k, a in want if k == "ncycle"]
    assert len(block) == len(plan_ncycle) == S
    for s in range(S):
        assert plan_ncycle[s].min() == 1 and 2 <= plan_ncycle[s].max() <= 3, (name, s, plan_ncycle[s])
        if n >= 2:
            assert block[s].min() == 1 and 2 <= block[s].max() <= 3, (name, s, block[s])
    if n == 1:
        per_step = [int(a[0]) for a in block]
        assert min(per_step) == 1 and 2 <= max(per_step) <= 3, (name, per_step)
    assert any(int(a.max()) == 3 for a in plan_ncycle), (name, plan_ncycle)


@pytest.fixture(scope="module")
def scripts(oracle, mpdata):
    """name -> (inputs, the script's records, the plan's ncycle per step), each computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            inputs = make_case(oracle, name)
            cache[name] = (inputs,) + replay(oracle, mpdata, name, inputs)
        return cache[name]
    return get


def _built():
    if not (shutil.which("amdflang") and all(os.path.exists(os.path.join(FDIR, o)) for o in ("mpdata_hip_mod.o", "mpdata_hip_mod.sp.o"))):
        pytest.skip("amdflang or the module's objects are missing (run __graft_entry__.build())")


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_subcycle_and_the_stream_round_trips(scripts, tmp_path, name):
    """(no GPU) the model alone: the condition on ncycle, and fortran_records.write_records / read_records are inverse"""
    inputs, want, plan_ncycle = scripts(name)
    check_subcycling(name, want, plan_ncycle)
    path = tmp_path / "records.bin"
    FR.write_records(path, want, end=True)
    back = FR.read_records(path)
    compare(back, want, name)
    if CASES[name]["tall"]:
        codes = {k: int(a[0]) for k, a in want if k.startswith("rc:diffuse")}
        assert codes and set(codes.values()) == {PM.EUNSUPPORTED}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_program_matches_the_models(scripts, tmp_path, name):
    inputs, want, plan_ncycle = scripts(name)
    check_subcycling(name, want, plan_ncycle)
    t0 = time.perf_counter()
    got = FR.run_program(EXE[CASES[name]["dt"]], list(inputs.items()), tmp_path)
    print(f"{name}: the program ran {time.perf_counter() - t0:.2f} s")
    compare(got, want, name)


# ------------------------------------------------------------------------------------------------ the module's text
def _c_functions():
    """name -> [(type, name)] of every function the header declares; type normalised: 'int64_t', 'int', 'double*', 'void**' ..."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(mpdata_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = re.sub(r"\bconst\b", "", p).strip()
            if p in ("void", ""):
                continue
            mm = re.match(r"(.*?)(\w+)$", p)
            params.append((mm.group(1).replace(" ", ""), mm.group(2)))
        out[m.group(1)] = params
    return out


def _module(text=None):
    """(macros, interfaces, public, contained) of the module's text.  macros: name -> (symbol under MPDATA_SINGLE, symbol
    otherwise); interfaces: Fortran name -> dict(bind = a macro name or a quoted symbol, args, decl = dummy -> (type, value?,
    assumed-size?)); public: the names of the public statements; contained: name -> body of every module procedure"""
    text = open(MODULE).read() if text is None else text
    text = re.sub(r"&[ \t]*\n[ \t]*&?", " ", text)
    code = "\n".join(line.split("!")[0] if not line.lstrip().startswith("#") else line for line in text.split("\n"))
    m = re.search(r"#ifdef MPDATA_SINGLE\n(.*?)#else\n(.*?)#endif", code, flags=re.S)
    single, double = (dict(re.findall(r'#define (\w+) "(\w+)"', part)) for part in m.groups())
    assert set(single) == set(double)
    macros = {k: (single[k], double[k]) for k in single}
    public = set()
    for line in re.findall(r"^\s*public\s*::(.*)$", code, flags=re.M | re.I):
        public |= {x.strip() for x in line.split(",")}
    for attrs, names in re.findall(r"^\s*integer\(c_int\)((?:\s*,\s*\w+)+)\s*::(.*)$", code, flags=re.M):
        if "public" in attrs:
            public |= {x.split("=")[0].strip() for x in names.split(",")}
    interfaces = {}
    block = re.search(r"^\s*interface\s*$(.*?)^\s*end interface", code, flags=re.S | re.M).group(1)
    for fm in re.finditer(r"^\s*(integer\(c_int\)|type\(c_ptr\)) function (\w+)\(([^)]*)\)\s*bind\(C, name=([^)]+)\)(.*?)^\s*end function",
                          block, flags=re.S | re.M):
        args = [a.strip() for a in fm.group(3).split(",") if a.strip()]
        decl = {}
        for line in fm.group(5).split("\n"):
            dm = re.match(r"\s*((?:integer|real|type)\(\w+\))((?:\s*,\s*[\w()]+)*)\s*::(.*)$", line)
            if not dm:
                assert not line.strip() or line.strip().startswith("import"), line
                continue
            attrs = [a.strip() for a in dm.group(2).split(",") if a.strip()]
            for ent in dm.group(3).split(","):
                ent = ent.strip()
                decl[ent.replace("(*)", "")] = (dm.group(1), "value" in attrs, ent.endswith("(*)"))
        interfaces[fm.group(2)] = dict(bind=fm.group(4).strip(), args=args, decl=decl, result=fm.group(1))
    contained = {}
    body = code.split("\ncontains\n", 1)[1]
    for pm in re.finditer(r"^\s*subroutine (\w+)\b(.*?)^\s*end subroutine", body, flags=re.S | re.M):
        contained[pm.group(1)] = pm.group(2)
    return macros, interfaces, public, contained


SCALARS = {"int64_t": "integer(c_int64_t)", "uint64_t": "integer(c_int64_t)", "int": "integer(c_int)"}
# fp64-only bindings of a function that has an _f32 sibling: the device-resident mode of the driver is fp64 (the module stops
# an MPDATA_SINGLE build that reaches it)
FP64_ONLY = {"mpdata_fill_synthetic_device"}


def _f32_sibling(cname, cfuncs):
    for cand in (cname + "_f32", cname[:-len("_device")] + "_f32_device" if cname.endswith("_device") else None):
        if cand in cfuncs:
            return cand
    return None


def kind_errors(text=None):
    """every disagreement between the module's interfaces and the header, as strings (an empty list: they agree)"""
    macros, interfaces, _, _ = _module(text)
    cfuncs = _c_functions()
    errors, seen = [], 0
    for fname, itf in interfaces.items():
        if itf["bind"].startswith('"'):
            cnames = {None: itf["bind"].strip('"')}
        else:
            if itf["bind"] not in macros:
                errors.append(f"{fname}: binds the unknown macro {itf['bind']}")
                continue
            sp, dp = macros[itf["bind"]]
            cnames = {"single": sp, "double": dp}
            if dp not in cfuncs or _f32_sibling(dp, cfuncs) != sp:
                errors.append(f"{fname}: {itf['bind']} names {sp} under MPDATA_SINGLE and {dp} otherwise; the header's pair is "
                              f"{_f32_sibling(dp, cfuncs)} / {dp}")
                continue
        for prec, cname in cnames.items():
            if cname not in cfuncs:
                errors.append(f"{fname}: {cname} is not in the header")
                continue
            seen += 1
            if prec is None and _f32_sibling(cname, cfuncs) and cname not in FP64_ONLY:
                errors.append(f"{fname}: binds {cname} in both precisions although the header has {_f32_sibling(cname, cfuncs)}")
            params = cfuncs[cname]
            if len(params) != len(itf["args"]):
                errors.append(f"{fname}: {len(itf['args'])} dummy arguments, {cname} has {len(params)}")
                continue
            real_of = {"single": "float*", "double": "double*"}
            for (ctype, cpar), arg in zip(params, itf["args"]):
                if arg not in itf["decl"]:
                    errors.append(f"{fname}: dummy argument {arg} has no declaration")
                    continue
                ftype, value, assumed = itf["decl"][arg]
                where = f"{fname}({arg}) against {cname}({ctype} {cpar})"
                if ctype in SCALARS:
                    ok = ftype == SCALARS[ctype] and value and not assumed
                elif ctype in ("mpdata_plan**", "void**"):
                    ok = ftype == "type(c_ptr)" and not value and not assumed
                elif ctype in ("mpdata_plan*", "void*"):
                    ok = ftype == "type(c_ptr)" and value
                elif ctype in ("double*", "float*"):
                    if ftype == "type(c_ptr)":
                        ok = value
                    elif ftype == "real(rp)":          # the module's precision: only behind a per-precision macro
                        ok = not value and prec is not None and ctype == real_of[prec]
                    else:
                        ok = ftype == "real(c_double)" and ctype == "double*" and not value
                elif ctype in ("int64_t*", "int*"):
                    ok = (ftype == "type(c_ptr)" and value) or (ftype == SCALARS[ctype[:-1]] and not value)
                else:
                    ok = False
                if not ok:
                    errors.append(f"{where}: declared {ftype}{', value' if value else ''}{' (*)' if assumed else ''}")
    assert seen >= 50, f"only {seen} bindings were compared: the parser has lost the interface block"
    return errors


def test_every_interface_matches_the_header_in_count_order_and_kind(mpdata):
    _built()
    assert kind_errors() == []
    macros, interfaces, _, _ = _module()
    L = mpdata.lib()
    for sp, dp in macros.values():                    # both names of every macro are exported
        assert hasattr(L, sp) and hasattr(L, dp), (sp, dp)
    # ... and in order by name as well: every dummy argument carries the name of the header's parameter
    cfuncs = _c_functions()
    for fname, itf in interfaces.items():
        cname = itf["bind"].strip('"') if itf["bind"].startswith('"') else macros[itf["bind"]][1]
        assert itf["args"] == [p for _, p in cfuncs[cname]], (fname, itf["args"], cfuncs[cname])
    # the calls of the header that had no interface before this test
    for fname in ("mpdata_plan_courant_c", "mpdata_courant_device_c", "mpdata_plan_run_uw_c", "mpdata_plan_run_tracers_c",
                  "mpdata_plan_set_stream_c", "mpdata_plan_set_timing_c"):
        assert fname in interfaces, fname


def test_the_kind_check_sees_a_wrong_kind():
    """the parser is not blind: three edits of the module's text, each of which must be reported"""
    _built()
    text = open(MODULE).read()
    anchor = 'bind(C, name="mpdata_plan_scale_uw_device")\n      import :: c_int, c_int64_t, c_ptr\n      type(c_ptr), value :: plan\n'
    assert text.count(anchor) == 1
    no_value = text.replace(anchor + "      integer(c_int64_t), value :: sl0, n\n",
                            anchor + "      integer(c_int64_t) :: sl0\n      integer(c_int64_t), value :: n\n")
    short_n = text.replace(anchor + "      integer(c_int64_t), value :: sl0, n\n",
                           anchor + "      integer(c_int64_t), value :: sl0\n      integer(c_int), value :: n\n")
    line = '#define MPDATA_C_PLAN_LEVEL_ADD "mpdata_plan_level_add_f32"'
    assert text.count(line) == 1
    fp64_name = text.replace(line, '#define MPDATA_C_PLAN_LEVEL_ADD "mpdata_plan_level_add"')
    for what, mutant in (("sl0 without value", no_value), ("n as c_int", short_n), ("the fp64 name under MPDATA_SINGLE", fp64_name)):
        assert mutant != text
        assert kind_errors(mutant), what


def _reachable_public():
    """(interfaces, public, what a program that `use`s the module reaches: the public names and everything the public module
    procedures call, through private ones as well)"""
    _, interfaces, public, contained = _module()
    reached, todo = set(public), [p for p in public if p in contained]
    while todo:
        for ident in set(re.findall(r"\b\w+\b", contained[todo.pop()])):
            if (ident in interfaces or ident in contained) and ident not in reached:
                reached.add(ident)
                if ident in contained:
                    todo.append(ident)
    return interfaces, public, reached


def test_every_interface_is_public_or_behind_a_public_wrapper():
    _built()
    interfaces, public, reached = _reachable_public()
    missing = sorted(n for n in interfaces if n not in reached)
    assert not missing, missing
    # the handle and the memory of a caller's own plan come from outside the module
    for n in ("mpdata_plan_create_c", "mpdata_plan_upload_c", "mpdata_plan_run_c", "mpdata_plan_sync_c", "mpdata_plan_download_c",
              "mpdata_plan_destroy_c", "mpdata_plan_import_device_c", "mpdata_plan_export_device_c",
              "mpdata_plan_import_instances_device_c", "mpdata_plan_export_instances_device_c", "mpdata_plan_download_instances_c",
              "mpdata_device_alloc_c", "mpdata_device_free_c", "mpdata_fill_synthetic_device_c", "mpdata_device_sum_c", "mpdata_last_error_c"):
        assert n in public, n


def test_integration_snippets_use_public_names():
    _built()
    _, _, public, _ = _module()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    part = doc.split("### 2b.")[1].split("\n## 3.")[0]
    assert "### 2c." in part
    fences = re.findall(r"```fortran\n(.*?)```", part, flags=re.S)
    assert len(fences) >= 9
    checked = 0
    for fence in fences:
        own = set(re.findall(r"function (mpdata_\w+)\(", fence)) | (set(re.findall(r"\buse (mpdata_\w+)", fence)) & {"mpdata_hip_mod", "mpdata_grid"})
        for ident in set(re.findall(r"\bmpdata_\w+", fence, flags=re.I)):
            if ident.upper() == ident:
                assert ident in public, f"INTEGRATION.md: {ident} is not a public name of the module"
            else:
                assert ident in public or ident in own, f"INTEGRATION.md: {ident} is not a public name of the module"
            checked += 1
    assert checked >= 15


def test_the_programs_are_built_and_bind_the_module_only():
    _built()
    macros, _, _, _ = _module()
    assert len(PROGRAMS) >= 7
    for dt, exe in ((dt, os.path.join(TDIR, prog + sfx)) for prog in PROGRAMS for dt, sfx in SUFFIX.items()):
        assert os.path.exists(exe), f"{exe}: not built (run __graft_entry__.build())"
        syms = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
        names = [line.split()[-1].split("@")[0] for line in syms.splitlines() if line.strip()]
        ours = [s for s in names if s.startswith(("mpdata_", "hip"))]
        assert not [s for s in names if "oracle" in s]
        assert {"hipMemcpy", "hipDeviceSynchronize", "mpdata_device_alloc", "mpdata_plan_run", "mpdata_plan_import_device"} <= set(ours)
        single = dt == np.float32
        for sp, dp in macros.values():
            if os.path.basename(exe) in EXE.values():      # plan_calls calls every interface; the others what their script needs
                assert (sp if single else dp) in ours, (exe, sp if single else dp)
            assert (dp if single else sp) not in ours, (exe, dp if single else sp)
        # nothing of the library is reached past the module: every mpdata_ symbol is one the module binds
        _, interfaces, _, _ = _module()
        bound = set()
        for itf in interfaces.values():
            bound |= {itf["bind"].strip('"')} if itf["bind"].startswith('"') else set(macros[itf["bind"]])
        # (_module reads the first interface block; the bindings with a real by value, 3p - 3r, stand in a second one)
        bound |= set(re.findall(r'bind\(C, name="(mpdata_\w+)"\)', open(MODULE).read()))
        assert {s for s in ours if s.startswith("mpdata_")} <= bound


# ------------------------------------------------------------------------------------------------ the build of the programs
@functools.lru_cache(maxsize=None)
def _dry_run(single):
    """the commands `make hip=1 [single=1]` runs from a clean tree, as lists of words: a dry run, nothing is compiled"""
    res = subprocess.run(["make", "-n", "-B", "hip=1"] + (["single=1"] if single else []), cwd=FDIR, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return [line.split() for line in res.stdout.replace("\\\n", " ").splitlines()]


@pytest.fixture(scope="module")
def ignored(tmp_path_factory):
    """path relative to the root -> does git ignore it by the project's .gitignore?  Asked of an empty repository that holds
    a copy of that file, so that the answer depends on the committed text alone and not on who owns the checkout"""
    repo = tmp_path_factory.mktemp("ignore")
    subprocess.run(["git", "init", "-q", str(repo)], check=True, capture_output=True)
    shutil.copy(os.path.join(ROOT, ".gitignore"), repo / ".gitignore")

    def ask(rel):
        code = subprocess.run(["git", "-C", str(repo), "check-ignore", "-q", "--no-index", rel], capture_output=True).returncode
        assert code in (0, 1), code
        return code == 0
    return ask


@pytest.mark.parametrize("dt", list(SUFFIX), ids=["f64", "f32"])
@pytest.mark.parametrize("prog", PROGRAMS)
def test_make_links_every_program_and_git_ignores_it(ignored, prog, dt):
    """every tests/fortran/*_calls.F90 has one link line that compiles it into its executable with the objects of
    mpdata_hip_mod, mpdata_grid and the shared module, and git ignores that executable (and not its source)"""
    single = dt == np.float32
    lines, o = _dry_run(single), ".sp.o" if single else ".o"
    exe = os.path.join(TDIR, prog + SUFFIX[dt])
    link = [w for w in lines if "-o" in w and w[w.index("-o") + 1] == exe]
    assert len(link) == 1, (exe, link)
    words = link[0]
    assert os.path.join(TDIR, prog + ".F90") in words and "-c" not in words, words
    for obj in ("mpdata_hip_mod" + o, "mpdata_grid" + o, COMMON + o):
        assert obj in words, (obj, words)
    assert ("-DMPDATA_SINGLE" in words) == single
    # the shared module is compiled once in this precision
    assert len([w for w in lines if "-c" in w and os.path.join(TDIR, COMMON + ".F90") in w and COMMON + o in w]) == 1
    assert ignored(f"tests/fortran/{prog}{SUFFIX[dt]}"), f"git does not ignore tests/fortran/{prog}{SUFFIX[dt]}"
    assert not ignored(f"tests/fortran/{prog}.F90")


def test_the_shared_text_of_the_programs_exists_once():
    """the helpers and the two HIP runtime interfaces are in one file; no program binds a C name itself"""
    texts = {p: open(p).read() for p in glob.glob(os.path.join(TDIR, "*.F90"))}
    for needle in ("subroutine expect", 'name="hipMemcpy"'):
        holders = [os.path.basename(p) for p, t in texts.items() if needle in t]
        assert holders == [COMMON + ".F90"], (needle, holders)
    assert len(PROGRAMS) >= 7
    for prog in PROGRAMS:
        assert "bind(C" not in texts[os.path.join(TDIR, prog + ".F90")], prog
