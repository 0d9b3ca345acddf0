"""oracle/plan_model.py -- TEST INFRASTRUCTURE: what a plan must hold after every call, and seeded call sequences.

`PlanModel` is the plan API of include/mpdata_hip.h sections 3, 3a, 3d, 3e, 3f restated on NumPy arrays and the CPU
oracle (oracle/oracle.py): the seven reference-layout arrays, the boundary mode and the flags `uploaded`, `have_u`,
`have_w`, `timing`, `ran` -- everything the header promises, and nothing the library keeps besides (layouts, tiles,
instance pairs, level windows, halo and seam bytes, the phantom half, shards: none of them is visible through the API,
which is what the sequences of tests/test_plan_sequences.py check).  It is written from the header, not from
mpdata_plan.hip.  Every method returns what the call must return -- None, or the arrays of a read-back -- or the
MPDATA_E* code the call must fail with; a failed call leaves the model unchanged.

f and flux always carry a trailing tracer axis here: f (ncrms, nx+6, nzm, T), flux (ncrms, nz, T).

`sequences(kind, seed, length)` draws one legal order of plan calls with concrete arguments for a plan kind of
`KINDS`; `fresh(kind, op)` makes the arrays an op hands over.  Only tests import this module.
"""
import numpy as np

EINVAL, EUNSUPPORTED, ESTATE = -1, -2, -3          # MPDATA_E* of include/mpdata_hip.h
GIVEN, PERIODIC = 0, 1                             # MPDATA_BOUNDARY_*
NAMES = ("f", "u", "w", "rho", "rhow", "adz", "flux")
MAX_STEPS = 8                                      # per tracer and sequence: ten steps keep max|f| below 1e3 on these inputs


def wrap(f):
    """f's halo columns -2..0, nx+1..nx+3 := column 1 + ((i-1) mod nx), in place (section 3a); idempotent"""
    nx = f.shape[1] - 6
    for i in (-2, -1, 0, nx + 1, nx + 2, nx + 3):
        f[:, i + 2] = f[:, 1 + (i - 1) % nx + 2]
    return f


class PlanModel:
    def __init__(self, oracle, ncrms, nx, nz, T, dtype):
        self.oracle, self.dims, self.dtype = oracle, (int(ncrms), int(nx), int(nz), int(T)), np.dtype(dtype).type
        sh = oracle.shapes(ncrms, nx, nz, 1)
        self.a = {k: np.zeros(sh[k] + ((T,) if k in ("f", "flux") else ()), self.dtype, order="F") for k in NAMES}
        self.boundary = GIVEN
        self.uploaded = self.have_u = self.have_w = False
        self.timing, self.ran = True, False
        # bookkeeping for the FAST bound of the GPU test, per tracer: steps taken, largest |f| and |flux(:, 1:nzm)| held
        self.steps = [0] * T
        self.fmax = [0.0] * T
        self.flmax = [0.0] * T

    # ---- helpers
    def _note(self):
        nzm = self.dims[2] - 1
        for t in range(self.dims[3]):
            self.fmax[t] = max(self.fmax[t], float(np.max(np.abs(self.a["f"][..., t]))))
            self.flmax[t] = max(self.flmax[t], float(np.max(np.abs(self.a["flux"][:, :nzm, t]))))

    def _wrap(self, first, count):
        if self.boundary == PERIODIC:
            wrap(self.a["f"][..., first:first + count])

    def _tracers_ok(self, first, count):
        return 0 <= first and 1 <= count and first + count <= self.dims[3]

    def _block_ok(self, sl0, n):
        return 0 <= sl0 and 1 <= n and sl0 + n <= self.dims[0]

    def finite(self):
        return all(bool(np.all(np.isfinite(a))) for a in self.a.values())

    def _step(self, u, w, first, count):
        nzm = self.dims[2] - 1
        self._wrap(first, count)
        sq = (lambda x: x[..., 0]) if count == 1 else (lambda x: x)
        inp = {k: self.a[k] for k in ("rho", "rhow", "adz")}
        inp.update(u=u, w=w, f=np.asfortranarray(sq(self.a["f"][..., first:first + count])),
                   flux=np.asfortranarray(sq(self.a["flux"][..., first:first + count])))
        f, flux = self.oracle.advect(inp, nthreads=4)
        self.a["f"][..., first:first + count] = f.reshape(self.a["f"].shape[:3] + (count,), order="F")
        self.a["flux"][:, :nzm, first:first + count] = flux.reshape(self.a["flux"].shape[:2] + (count,), order="F")[:, :nzm]
        for t in range(first, first + count):
            self.steps[t] += 1
        self._note()

    def _put(self, sl0, n, arrs, first, ntr):
        for k, v in arrs.items():
            if k in ("f", "flux"):
                self.a[k][sl0:sl0 + n, ..., first:first + ntr] = v.reshape((n,) + self.a[k].shape[1:-1] + (ntr,), order="F")
            else:
                self.a[k][sl0:sl0 + n] = v
        self._note()

    def _get(self, sl0, n, what, first, ntr):
        if "f" in what:
            self._wrap(first, ntr)
        return {k: np.array(self.a[k][sl0:sl0 + n, ..., first:first + ntr], order="F") for k in what}

    # ---- section 3: whole imports
    def upload(self, arrs):
        """all seven host arrays (flux may be left out: zeros)"""
        if any(k not in arrs for k in NAMES[:6]):
            return EINVAL
        arrs = dict(arrs)
        arrs.setdefault("flux", np.zeros_like(self.a["flux"]))
        return self.import_device(arrs, 0, self.dims[3])

    def import_device(self, arrs, first=0, ntr=None):
        ntr = self.dims[3] if ntr is None else ntr
        if not arrs or not self._tracers_ok(first, ntr):
            return EINVAL
        self._put(0, self.dims[0], arrs, first, ntr)
        self.have_u = self.have_u or "u" in arrs      # u and w count separately (section 3, mpdata_plan_run_uw)
        self.have_w = self.have_w or "w" in arrs
        self.uploaded = True
        return None

    # ---- section 3d: blocks of instances
    def import_block(self, sl0, n, arrs, first=0, ntr=None):
        ntr = self.dims[3] if ntr is None else ntr
        if not arrs or not self._block_ok(sl0, n) or not self._tracers_ok(first, ntr):
            return EINVAL
        if not self.uploaded or ("u" in arrs and not self.have_u) or ("w" in arrs and not self.have_w):
            return ESTATE
        self._put(sl0, n, arrs, first, ntr)
        return None

    # ---- runs
    def run(self, first=None, count=None):
        first, count = (0, self.dims[3]) if first is None else (first, 1 if count is None else count)
        if not self._tracers_ok(first, count):
            return EINVAL
        if not (self.uploaded and self.have_u and self.have_w):
            return ESTATE
        self._step(self.a["u"], self.a["w"], first, count)
        self.ran = self.timing
        return None

    def run_uw(self, u, w, first=0, count=None):
        count = self.dims[3] - first if count is None else count
        if not self._tracers_ok(first, count):
            return EINVAL
        if not self.uploaded:
            return ESTATE
        self._step(u, w, first, count)
        self.have_u = self.have_w = False    # the post-condition, on every path; the plan's own u, w are not promised
        self.ran = self.timing
        return None

    # ---- section 3a
    def set_boundary(self, mode):
        if mode not in (GIVEN, PERIODIC):
            return EINVAL
        if self.boundary == PERIODIC and mode == GIVEN:
            self._wrap(0, self.dims[3])   # "the plan then holds what an export just before the switch would have returned"
        self.boundary = mode
        return None

    # ---- read-backs: {name: array} of the arrays asked for
    def export_device(self, what=("f", "flux"), first=0, ntr=None):
        ntr = self.dims[3] if ntr is None else ntr
        if not what or not self._tracers_ok(first, ntr):
            return EINVAL
        return self._get(0, self.dims[0], what, first, ntr) if self.uploaded else ESTATE

    def export_block(self, sl0, n, what=("f", "flux"), first=0, ntr=None):
        ntr = self.dims[3] if ntr is None else ntr
        if not what or not self._block_ok(sl0, n) or not self._tracers_ok(first, ntr):
            return EINVAL
        return self._get(sl0, n, what, first, ntr) if self.uploaded else ESTATE

    def download(self, what=("f", "flux")):
        return self.export_device(what)

    def download_block(self, sl0, n, what=("f", "flux")):
        return self.export_block(sl0, n, what)

    # ---- timing (mpdata_plan_set_timing: the pair is recorded around every run while it is on; switched off,
    # last_kernel_ms returns MPDATA_ESTATE -- until a run has been recorded with the pair on again)
    def set_timing(self, on):
        self.timing = bool(on)
        if not on:
            self.ran = False
        return None

    def last_kernel_ms(self):
        return True if self.ran else ESTATE

    def set_stream(self):
        return None

    def sync(self):
        return None


# ------------------------------------------------------------------------------------------------- plan kinds
def _k(shape, dtype="f64", **sw):
    return dict(dict(shape=shape, dtype=dtype, ref=False, tall=False, odd=False, multi=0), **sw)


# the smallest shapes at which each path of the library exists: (ncrms, nx, nz, T), precision, the switches to set
KINDS = {
    "ref": _k((5, 6, 12, 3), ref=True),                       # reference-layout plan, slab block copies
    "wm8": _k((17, 5, 7, 2)), "wm16": _k((9, 5, 16, 2)),      # every LPS, the last tile padded
    "wm32": _k((7, 6, 28, 3)), "wm64": _k((3, 6, 58, 2)),
    "wm-ring-t1": _k((6, 6, 28, 1)), "wm-ring-t3": _k((6, 6, 28, 3)),   # run_uw kernels that read the caller's u, w
    "wm-park": _k((3, 70, 28, 2)),                            # EXACT park array (nx > 66), allocated by the first run_uw
    "ks-72": _k((3, 5, 72, 2)), "ks-128": _k((3, 5, 128, 2)),  # several waves per instance: tail wave / whole waves
    "f32-28": _k((6, 6, 28, 2), "f32"), "f32-72": _k((4, 5, 72, 2), "f32"),   # packed pairs, blocks that split them
    "f32-odd-28": _k((5, 6, 28, 2), "f32", odd=True), "f32-odd-72": _k((3, 5, 72, 2), "f32", odd=True),
    "f32-odd-16": _k((1, 5, 16, 1), "f32", odd=True),         # the phantom half through every call
    "tall-239": _k((3, 5, 239, 2), tall=True), "tall-300": _k((2, 6, 300, 2), tall=True),   # the seam byte
    "tall-f32": _k((4, 5, 300, 2), "f32", tall=True),         # pairs of pseudo-instances
    "tall-f32-odd-239": _k((3, 5, 239, 2), "f32", tall=True, odd=True),   # 15 pseudo-instances: an inner phantom
    "tall-f32-odd-300": _k((5, 3, 300, 2), "f32", tall=True, odd=True),   # 30: none
    "multi-28": _k((7, 5, 28, 2), multi=2), "multi-300": _k((7, 5, 300, 2), tall=True, multi=2),   # two shards
}
# three seeds per kind, the first whose sequences meet every condition of tests/test_plan_model_cpu.py (a seed that
# misses one is replaced here, the conditions stay); FAST plays the first of each
SEEDS = {
    "ref": (5, 9, 11), "wm8": (5, 11, 13), "wm16": (4, 5, 6), "wm32": (8, 9, 14), "wm64": (1, 4, 6),
    "wm-ring-t1": (2, 3, 9), "wm-ring-t3": (2, 4, 6), "wm-park": (7, 10, 12), "ks-72": (4, 5, 7), "ks-128": (1, 3, 4),
    "f32-28": (3, 4, 12), "f32-72": (6, 7, 9), "f32-odd-28": (4, 7, 8), "f32-odd-72": (5, 6, 12), "f32-odd-16": (2, 4, 10),
    "tall-239": (4, 8, 12), "tall-300": (3, 6, 8), "tall-f32": (2, 5, 6), "tall-f32-odd-239": (1, 10, 17),
    "tall-f32-odd-300": (1, 2, 3), "multi-28": (3, 4, 5), "multi-300": (3, 4, 7),
}
LENGTH = 14
DTYPES = {"f64": np.float64, "f32": np.float32}


def shard_ranges(ncrms, ngpus):
    """contiguous blocks, the remainder on the low shards (mpdata_shard_range)"""
    out, a = [], 0
    for g in range(ngpus):
        n = ncrms // ngpus + (1 if g < ncrms % ngpus else 0)
        out.append((a, n))
        a += n
    return out


def fresh(kind, op, oracle=None):
    """the arrays op hands over, {name: array}: oracle.make_inputs of the op's instances with the op's seed,
    conditioned law; tracer t of f / flux from seed + 7 t / seed + 11 t; f and flux with a tracer axis"""
    if oracle is None:
        from . import oracle
    ncrms, nx, nz, T = KINDS[kind]["shape"]
    dt = DTYPES[KINDS[kind]["dtype"]]
    n, ntr, seed = op.get("n", ncrms), op.get("ntr", T), op["seed"]
    mk = lambda s: oracle.make_inputs(n, nx, nz, seed=s, dist=oracle.DIST_CONDITIONED, dtype=dt)
    base, out = mk(seed), {}
    for k in op["names"]:
        if k in ("f", "flux"):
            step = 7 if k == "f" else 11
            out[k] = np.asfortranarray(np.stack([(base if t == 0 else mk(seed + step * t))[k] for t in range(ntr)], axis=-1))
        else:
            out[k] = base[k]
    return out


def apply(model, kind, op, oracle=None):
    """play op on the model; returns what the model's method returns"""
    o = op["op"]
    if o == "upload":
        return model.upload(fresh(kind, op, oracle))
    if o == "import_device":
        return model.import_device(fresh(kind, op, oracle), op["first"], op["ntr"])
    if o == "import_block":
        return model.import_block(op["sl0"], op["n"], fresh(kind, op, oracle), op["first"], op["ntr"])
    if o == "run":
        return model.run(op.get("first"), op.get("count"))
    if o == "run_uw":
        a = fresh(kind, dict(op, names=("u", "w")), oracle)
        return model.run_uw(a["u"], a["w"], op["first"], op["count"])
    if o == "set_boundary":
        return model.set_boundary(op["mode"])
    if o == "export_device":
        return model.export_device(op["what"], op["first"], op["ntr"])
    if o == "export_block":
        return model.export_block(op["sl0"], op["n"], op["what"], op["first"], op["ntr"])
    if o == "download":
        return model.download()
    if o == "download_block":
        return model.download_block(op["sl0"], op["n"], op["what"])
    if o == "timing":     # set_timing(on), then the probe: the probe's result
        model.set_timing(op["on"])
        return model.last_kernel_ms()
    if o == "set_stream":
        return model.set_stream()
    if o == "sync":
        return model.sync()
    if o == "handle_block":   # a block call on a multi-GPU handle
        return EUNSUPPORTED
    raise ValueError(o)


# op classes every sequence holds at least once, and what else is drawn
_MUST = ("import_device", "import_block", "run_sub", "run_uw", "set_boundary", "export_device", "export_block", "download",
         "download_block", "run", "run")
_ANY = ("import_device", "import_block", "import_block", "run", "run", "run_sub", "run_uw", "set_boundary", "export_device",
        "export_block", "download", "download_block", "set_stream", "timing", "timing")


def sequences(kind, seed, length=LENGTH, oracle=None):
    """The ops of sequence `seed` on plan kind `kind`: a whole fill, `length` drawn ops, then sync, a whole
    export_device and a whole download.  Deterministic.  Ops are plain dicts (a printed list replays).  The model is
    played along: an op the model refuses stays in the list with the code it must raise under "err"."""
    if oracle is None:
        from . import oracle
    spec = KINDS[kind]
    ncrms, nx, nz, T = spec["shape"]
    rng = np.random.default_rng([seed, sorted(KINDS).index(kind)])
    model = PlanModel(oracle, ncrms, nx, nz, T, DTYPES[spec["dtype"]])
    shards = shard_ranges(ncrms, spec["multi"]) if spec["multi"] else [(0, ncrms)]
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))     # inclusive
    deck = list(_MUST) + [_ANY[ri(0, len(_ANY) - 1)] for _ in range(max(0, length - len(_MUST)))]
    if spec["multi"]:
        deck[len(_MUST)] = "handle_block"
    deck = [deck[i] for i in rng.permutation(len(deck))][:length]
    patterns = [("tail", "odd", "one", "split")[i] for i in rng.permutation(4)]
    ops, stream_is_new = [], False

    def tracers():
        first = ri(0, T - 1)
        return first, ri(1, T - first)

    def block():
        """(shard, global sl0, n) after the next pattern: ends on the last instance / odd sl0 / one instance / splits a
        pair of adjacent instances at both ends; where the shard is too small for a pattern, the nearest legal block"""
        pat = patterns.pop(0) if patterns else ("tail", "odd", "one", "split", "any")[ri(0, 4)]
        g = len(shards) - 1 if pat == "tail" else ri(0, len(shards) - 1)
        base, m = shards[g]
        if pat == "tail":
            n = ri(1, m)
            sl0 = m - n
        elif pat == "one":
            n, sl0 = 1, ri(0, m - 1)
        elif pat == "odd" and m >= 2:
            sl0 = 2 * ri(0, (m - 2) // 2) + 1
            n = ri(1, m - sl0)
        elif pat == "split" and m >= 3:
            sl0 = 2 * ri(0, (m - 3) // 2) + 1
            n = 2 * ri(1, (m - sl0) // 2)          # sl0 and sl0 + n odd: the pairs at both ends are split
        else:
            sl0 = ri(0, m - 1)
            n = ri(1, m - sl0)
        return g, base + sl0, n

    def data_seed():
        return 100000 + 1009 * seed + 31 * len(ops)

    def draw(cls):
        nonlocal stream_is_new
        if cls == "import_device":
            k = ri(1, 7)
            names = [NAMES[i] for i in sorted(rng.permutation(7)[:k])]
            if not (model.have_u and model.have_w):   # after run_uw: mostly hand both back, sometimes u alone
                r = rng.random()
                names = sorted(set(names) | {"u", "w"}, key=NAMES.index) if r < 0.6 else (["u"] if r < 0.8 else names)
            first, ntr = tracers()
            return dict(op="import_device", names=names, first=first, ntr=ntr, seed=data_seed())
        if cls == "import_block":
            g, sl0, n = block()
            k = ri(1, 4)
            names = [NAMES[i] for i in sorted(rng.permutation(7)[:k])]
            if rng.random() < 0.5 and "f" not in names:
                names = ["f"] + names
            first, ntr = tracers()
            return dict(op="import_block", shard=g, sl0=sl0, n=n, names=names, first=first, ntr=ntr, seed=data_seed())
        if cls in ("run", "run_sub", "run_uw"):
            first, count = (0, T) if cls == "run" or (cls == "run_uw" and rng.random() < 0.5) else tracers()
            if max(model.steps[first:first + count]) >= MAX_STEPS:
                return draw("export_device")
            if cls == "run":
                return dict(op="run")
            if cls == "run_sub":
                return dict(op="run", first=first, count=count)
            return dict(op="run_uw", first=first, count=count, seed=data_seed())
        if cls == "set_boundary":
            return dict(op="set_boundary", mode=1 - model.boundary)
        what = [["f", "flux"], ["f", "flux"], ["f"], ["flux"]][ri(0, 3)]
        if cls == "export_device":
            first, ntr = tracers()
            return dict(op="export_device", what=what, first=first, ntr=ntr)
        if cls in ("export_block", "handle_block"):
            g, sl0, n = block()
            first, ntr = tracers()
            return dict(op=cls, shard=g, sl0=sl0, n=n, what=what, first=first, ntr=ntr)
        if cls == "download":
            return dict(op="download")
        if cls == "download_block":
            g, sl0, n = block()
            return dict(op="download_block", shard=g, sl0=sl0, n=n, what=what)
        if cls == "set_stream":
            if spec["multi"]:          # (a multi-GPU plan runs on its own streams)
                return draw("timing")
            stream_is_new = not stream_is_new or rng.random() < 0.3
            return dict(op="set_stream", new=bool(stream_is_new))
        if cls == "timing":
            return dict(op="timing", on=int(not model.timing))
        raise ValueError(cls)

    def play(op):
        r = apply(model, kind, op, oracle)
        if isinstance(r, int) and not isinstance(r, bool):
            op["err"] = r
        ops.append(op)
        assert model.finite(), f"{kind} seed {seed}: the model is not finite after op {len(ops) - 1}: {ops}"

    play(dict(op=("upload", "import_device")[ri(0, 1)], names=list(NAMES), first=0, ntr=T, seed=data_seed()))
    for cls in deck:
        play(draw(cls))
    play(dict(op="sync"))
    play(dict(op="export_device", what=["f", "flux"], first=0, ntr=T))
    play(dict(op="download"))
    return ops
