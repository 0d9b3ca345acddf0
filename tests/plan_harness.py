"""What the GPU tests of the in-place calls on a resident plan share (tests/test_plan_*.py): the fixture that puts the
library's switches back, the device buffers with guard bands, the helpers that make a plan of a kind and compare its
whole export with a plan model, and the driver of the seeded call sequences (tests/test_plan_<call>_sequences.py).

A new call's sequence test starts here: its file keeps CASES, STEPS, OPS, the script prefix, the Model mix-in, the
handlers of the call under test and the final count assertions, and hands them to Sequence.play.  (The Player family of
tests/test_plan_sequences.py plays sequences that oracle/plan_model.py draws; it is another design and not served here.)"""
import numpy as np
import pytest

import cell_add_model as CM
import diffuse_model as DM
import level_add_model as AM
import sediment_model as SM
import subside_model as UM
import vsolve_model as VM
from oracle import plan_model as PM
from util import assert_bitwise, to_dev, to_host

BAND = 4096


# ---- a. the library's defaults before and after every test of a module that imports the fixture
def reset_defaults(mpdata):
    mpdata.set_tile(-1)
    mpdata.set_wm_flags(0)
    mpdata.set_plan_layout(mpdata.LAYOUT_WAVEMAJOR)
    mpdata.set_variant(mpdata.VARIANT_EXACT)
    mpdata.set_tall_columns(0)
    mpdata.set_f32_odd_ncrms(0)


@pytest.fixture(autouse=True)
def _defaults(mpdata):
    reset_defaults(mpdata)
    yield
    reset_defaults(mpdata)


# ---- b. device buffers and whole-plan helpers
def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def upload(p, inp):
    p.upload(inp["f"], inp["u"], inp["w"], inp["rho"], inp["rhow"], inp["adz"], inp["flux"])


def banded(shape, dt):
    """(raw bytes, pristine copy, view of `shape` between two bands of BAND patterned bytes)"""
    import torch
    nb = int(np.prod(shape)) * np.dtype(dt).itemsize
    raw = (torch.arange(nb + 2 * BAND, device="cuda:0") % 251).to(torch.uint8)
    return raw, raw.clone(), raw[BAND:BAND + nb].view(tdt(dt)).view(tuple(shape))


def bands_kept(raw, pristine):
    import torch
    return torch.equal(raw[:BAND], pristine[:BAND]) and torch.equal(raw[-BAND:], pristine[-BAND:])


def nan_banded(a, shape):
    """host array a -> (raw, view of torch `shape`): the bytes of a between two bands of BAND bytes of NaN"""
    import torch
    t = to_dev(a).reshape(-1)
    pad = BAND // t.element_size()
    raw = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device="cuda:0")
    raw[pad:pad + t.numel()] = t
    return raw, raw[pad:pad + t.numel()].view(tuple(shape))


def nan_out(shape, dt):
    """banded(shape, dt) with every element of the view NaN"""
    raw, pristine, view = banded(shape, dt)
    view.fill_(float("nan"))
    return raw, pristine, view


def new_plan(M, kind, name, ref, windows, variant=None):
    """the plan of kind = (shape, tracers, dtype, switches), made under its switches.  ref: the plan must come out in the
    reference layout -- the caller says so, the switches do not: an odd fp32 plan without the opt-in, or one above 238
    levels without tall columns, lands there although nothing asks for it.  windows: True / False: the plan must / must
    not be one of level windows; None: not asserted."""
    shape, T, dt, sw = kind
    M.set_variant(M.VARIANT_EXACT if variant is None else variant)
    M.set_plan_layout(M.LAYOUT_REFERENCE if sw.get("ref") else M.LAYOUT_WAVEMAJOR)
    M.set_tall_columns(int(bool(sw.get("tall"))))
    M.set_f32_odd_ncrms(int(bool(sw.get("odd"))))
    p = M.Plan(*shape, T, dtype=dt)
    assert p.layout == (M.LAYOUT_REFERENCE if ref else M.LAYOUT_WAVEMAJOR), name
    assert windows is None or (p.level_windows > 1) == windows, name
    return p


def whole(M, p, kind, what=("f", "flux")):
    """the plan's whole export -> {name: Fortran array WITH a tracer axis}"""
    import torch
    shape, T, dt, _ = kind
    sh = M.shapes(*shape, T)
    t = {k: torch.empty(sh[k], dtype=tdt(dt), device="cuda:0") for k in what}
    p.export_device(**t)
    p.sync()
    return {k: to_host(v).reshape(to_host(v).shape + (() if T > 1 else (1,)), order="F") for k, v in t.items()}


def same_as_model(M, p, kind, name, m, what):
    got, want = whole(M, p, kind), m.export_device()
    for k in ("f", "flux"):
        assert_bitwise(got[k], want[k], f"{name} {what}: {k}")


# ---- c. seeded call sequences on a plan and its model, side by side
class Sequence:
    """A resident plan `p` of one kind and the plan model `m` with the same arrays, and the seeded generator `rng` that
    every draw of the sequence comes from -- which ops run, on which blocks, with which arrays is a function of the ORDER
    of the draws, so: the script is completed first, block() is drawn once per step ahead of the handler whether the op
    uses it or not, and a handler draws what its text draws, in that order.

    name, kind = (shape, tracers, dtype, switches), seed: the case.  Model: the file's mix-in class; make_inputs: its
    make_plan_inputs.  ref, windows: the layout and the level windows the plan must come out with (new_plan).
    periodic: the plan and the model are PERIODIC from the start."""

    def __init__(self, M, oracle, Model, make_inputs, name, kind, seed, ref, windows, periodic=False):
        self.M, self.oracle, self.name, self.kind, self.seed = M, oracle, name, kind, seed
        self.shape, self.T, self.dt, self.sw = kind
        self.ncrms, self.nx, self.nz = self.shape
        self.p = new_plan(M, kind, name, ref, windows)
        self.inp = make_inputs(oracle, self.shape, self.T, self.dt, 100 + seed)
        upload(self.p, self.inp)
        self.m = Model(oracle, *self.shape, self.T, self.dt)
        self.m.windowed = bool(self.sw.get("tall"))     # (read by the models of diffuse and column_step, which refuse)
        assert self.m.upload({k: np.array(v, order="F") for k, v in self.inp.items()}) is None
        if periodic:
            self.p.set_boundary(M.BOUNDARY_PERIODIC)
            assert self.m.set_boundary(PM.PERIODIC) is None
        self.rng = np.random.default_rng(seed)
        self.i, self.op, self.count = 0, None, {}

    def block(self):
        rng, ncrms, T = self.rng, self.ncrms, self.T
        sl0 = int(rng.integers(0, ncrms))
        n = int(rng.integers(1, ncrms - sl0 + 1))
        if rng.random() < 0.3:
            sl0, n = 0, ncrms
        first = int(rng.integers(0, T))
        return sl0, n, first, int(rng.integers(1, T - first + 1))

    def fresh_f(self, n, ntr, s):
        O, dt = self.oracle, self.dt
        per = [O.make_inputs(n, self.nx, self.nz, seed=1000 * self.seed + 10 * s + t, dist=O.DIST_RAW_SIGNED, dtype=dt)["f"] - dt(0.5)
               for t in range(ntr)]
        return per[0] if ntr == 1 else np.asfortranarray(np.stack(per, axis=-1))

    def code(self, fn, *a, **kw):
        """the call's return code: None, or the code of the MpdataError it raises"""
        try:
            fn(*a, **kw)
        except self.M.MpdataError as e:
            return e.code
        return None

    def export(self):
        import torch
        t = {k: torch.empty(self.M.shapes(*self.shape, self.T)[k], dtype=tdt(self.dt), device="cuda:0") for k in ("f", "flux")}
        assert self.code(self.p.export_device, **t) is None
        self.p.sync()
        want = self.m.export_device()
        for k in t:
            assert_bitwise(to_host(t[k]), want[k], f"{self.name} step {self.i}: export of {k}")

    def seed_of_step(self):
        return self.seed * 100 + self.i

    def at(self, what, sl0, n, first, ntr):
        """a step's message"""
        return f"{self.name} step {self.i}: {what} of block {sl0, n} tracers {first, ntr}"

    def play(self, prefix, ops, steps, handlers, after=None):
        """Completes the script prefix to `steps` ops drawn from `ops`, plays it and compares the final export; -> the
        count of every op.  A handler is f(seq, sl0, n, first, ntr): handlers[op] where the file gives one (the call
        under test), else the plain form PLAIN[op].  after(seq): called behind every step's m.finite()."""
        script = list(prefix) + [str(self.rng.choice(ops)) for _ in range(steps - len(prefix))]
        self.count = dict.fromkeys(ops, 0)
        table = {op: handlers[op] if op in handlers else PLAIN[op] for op in ops}
        for i, op in enumerate(script):
            self.i, self.op = i, op
            self.count[op] += 1
            blk = self.block()
            table[op](self, *blk)
            assert self.m.finite()
            if after is not None:
                after(self)
        self.i = len(script)
        self.export()
        self.p.close()
        return self.count


def _run(s, sl0, n, first, ntr):
    assert s.code(s.p.run) is None and s.m.run() is None


def run_tracers(s, sl0, n, first, ntr):
    assert s.code(s.p.run, first, ntr) is None and s.m.run(first, ntr) is None


def _export(s, sl0, n, first, ntr):
    s.export()


def _export_block(s, sl0, n, first, ntr):
    import torch
    t = torch.empty(s.M.shapes(n, s.nx, s.nz, ntr)["f"], dtype=tdt(s.dt), device="cuda:0")
    assert s.code(s.p.export_block, sl0, f=t, first_tracer=first) is None
    s.p.sync()
    want = s.m.export_block(sl0, n, ("f",), first, ntr)["f"]
    assert_bitwise(to_host(t).reshape(want.shape, order="F"), want, f"{s.name} step {s.i}: export of block {sl0, n}")


def _set_boundary(s, sl0, n, first, ntr):
    mode = 1 - s.m.boundary
    assert s.code(s.p.set_boundary, mode) is None and s.m.set_boundary(mode) is None
    assert s.p.boundary == mode


def _import(s, sl0, n, first, ntr):
    f = s.fresh_f(s.ncrms, ntr, s.i)
    assert s.code(s.p.import_device, f=to_dev(f), first_tracer=first) is None
    assert s.m.import_device({"f": f}, first, ntr) is None


def _import_block(s, sl0, n, first, ntr):
    f = s.fresh_f(n, ntr, s.i)
    assert s.code(s.p.import_block, sl0, f=to_dev(f), first_tracer=first) is None
    assert s.m.import_block(sl0, n, {"f": f}, first, ntr) is None


def _level_add(s, sl0, n, first, ntr):
    S = float(np.max(np.abs(s.m.a["f"][sl0:sl0 + n, ..., first:first + ntr])))
    d = np.asfortranarray((s.rng.uniform(-1.0, 1.0, (n, s.nz - 1, ntr)) * S).astype(s.dt))
    assert s.code(s.p.level_add, to_dev(d), sl0, n, AM.ADD, first) is None
    assert s.m.level_add(d, sl0, n, AM.ADD, first) is None


def _subside(s, sl0, n, first, ntr):
    cb, cc = UM.make_coeffs(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.subside, to_dev(cb), to_dev(cc), None, sl0, n, first, ntr) is None
    assert s.m.subside(cb, cc, sl0=sl0, n=n, first=first, ntr=ntr) is not None


def _sediment(s, sl0, n, first, ntr):
    wp = SM.make_wp(n, s.nx, s.nz, ntr, s.dt, s.seed_of_step())
    assert s.code(s.p.sediment, to_dev(wp), None, None, sl0, n, first, ntr) is None
    assert not isinstance(s.m.sediment(wp, sl0=sl0, n=n, first=first, ntr=ntr), int)


def _vsolve(s, sl0, n, first, ntr):
    lo, di, up = VM.make_coeffs(n, s.nz, s.dt, s.seed_of_step())
    assert s.code(s.p.vsolve, to_dev(lo), to_dev(di), to_dev(up), sl0, n, first, ntr) is None
    assert s.m.vsolve(lo, di, up, sl0=sl0, n=n, first=first, ntr=ntr) is None


def _diffuse(s, sl0, n, first, ntr):
    """a windowed plan refuses, and the model with it"""
    c = DM.make_coeffs(n, s.nx, s.nz, s.dt, s.seed_of_step())
    dev = {k: None if v is None else to_dev(v) for k, v in c.items()}
    got = s.code(s.p.diffuse, dev["tkh"], dev["cx"], dev["cz"], dev["sb"], dev["st"], None, sl0, n, first, ntr)
    want = s.m.diffuse(c["tkh"], c["cx"], c["cz"], c["sb"], c["st"], sl0=sl0, n=n, first=first, ntr=ntr)
    assert got == (want if isinstance(want, int) else None), (got, want)
    assert (got == s.M.EUNSUPPORTED) == bool(s.sw.get("tall"))


# the plain form of every common op: no output asked for, plain device inputs, only the return codes compared
PLAIN = {"run": _run, "run_tracers": run_tracers, "export": _export, "export_block": _export_block, "set_boundary": _set_boundary,
         "import": _import, "import_block": _import_block, "level_add": _level_add, "subside": _subside, "sediment": _sediment,
         "vsolve": _vsolve, "diffuse": _diffuse}


def plain_cell_add(c):
    """the plain form of cell_add (ADD) with the factor c, which is the file's"""
    def cell_add(s, sl0, n, first, ntr):
        a = CM.make_s(n, s.nx, s.nz, ntr, s.dt, s.seed_of_step())
        assert s.code(s.p.cell_add, to_dev(a), c, CM.ADD, None, sl0, n, first, ntr) is None
        assert not isinstance(s.m.cell_add(a, c, CM.ADD, sl0=sl0, n=n, first=first, ntr=ntr), int)
    return cell_add


def checked_sediment(s, sl0, n, first, ntr):
    """sediment as a call under test: wp between NaN bands; psfc and pflux, each asked for with probability 0.7 (up to
    two draws), NaN-filled between patterned bands and compared with the model's"""
    import torch
    wp = SM.make_wp(n, s.nx, s.nz, ntr, s.dt, s.seed_of_step())
    outs = [k for k in ("psfc", "pflux") if s.rng.random() < 0.7]
    sh = s.M.sediment_shapes(n, s.nx, s.nz, ntr)
    wraw, wview = nan_banded(wp, sh["wp"])
    bufs = {k: nan_out(sh[k], s.dt) for k in outs}
    torch.cuda.synchronize()
    assert s.code(s.p.sediment, wview, bufs["psfc"][2] if "psfc" in bufs else None, bufs["pflux"][2] if "pflux" in bufs else None,
                  sl0, n, first, ntr) is None
    s.p.sync()
    want = dict(zip(("psfc", "pflux"), s.m.sediment(wp, sl0=sl0, n=n, first=first, ntr=ntr)))
    for k, (raw, pristine, view) in bufs.items():
        assert bands_kept(raw, pristine)
        assert_bitwise(to_host(view), want[k], s.at(k, sl0, n, first, ntr))
