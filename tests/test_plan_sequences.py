"""GPU tests: seeded call sequences on every kind of plan against the plan model (oracle/plan_model.py).

A plan's state shows only across calls -- `uploaded`, `have_u` / `have_w`, the per-tracer halo and seam bytes, the
phantom half of odd fp32 plans, the serpentine counter, the lazily allocated park array, `ran` / `timing`, the boundary
mode and the stream a windowed plan forwards to its inner plan -- and a stale flag does not fault: it returns a
plausible field.  Each case plays one sequence of PM.sequences (a whole fill, 14 drawn ops, sync, whole export_device,
whole download) on a real Plan and on the model side by side:
  * an op the model refuses must raise MpdataError with the model's code, and changes nothing (the next read-back
    still equals the model);
  * every read-back, EXACT: bit for bit the model's arrays -- f with its halo columns, flux at all nz levels; the
    targets are pre-filled with a NaN pattern, so an element that was not written shows;
  * every read-back, FAST: per tracer max|f - f_model| <= K * 64 u * S, K the steps that tracer has taken so far, S the
    largest |f| it has held in the model so far; the same on flux(:, 1:nzm) against the largest model |flux|;
    flux(:, nz) bit for bit (the library's FAST bound, include/mpdata_hip.h MPDATA_VARIANT_FAST, scaled by the step
    count as tests/test_plan_tall_columns.py scales it);
  * the final whole export_device and whole download agree bit for bit, in both variants;
  * arrays handed to imports and to run_uw are bit-identical afterwards.
Device read-backs and the inputs are compared at the sequence's own synchronisation points (sync, download,
set_stream), so the test adds no synchronisation of its own between asynchronous calls.  A failure names the kind, the
seed, the op index and prints the ops up to there as a list that replays; nothing is retried.
"""
import json

import numpy as np
import pytest

from oracle import plan_model as PM
from plan_harness import _defaults
from test_plan_tall_columns import UNIT, C_FAST, w_of
from util import assert_bitwise, to_dev, to_host

pytestmark = pytest.mark.gpu

CASES = [(k, s, "exact") for k in PM.KINDS for s in PM.SEEDS[k]] + [(k, PM.SEEDS[k][0], "fast") for k in PM.KINDS]
NAN_BITS = {np.float64: (np.uint64, 0x7FF8DEADBEEF0000), np.float32: (np.uint32, 0x7FC0DEAD)}


@pytest.fixture(scope="module")
def M(mpdata):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    return mpdata


def unwritten(shape, dt):
    ui, bits = NAN_BITS[dt]
    return np.full(shape, bits, ui, order="F").view(dt)


def squeeze(a, name):
    """the library's arrays have no tracer axis for one tracer"""
    return np.asfortranarray(a[..., 0]) if name in ("f", "flux") and a.shape[-1] == 1 else a


class Player:
    def __init__(self, M, oracle, kind, variant):
        import torch
        self.torch, self.M, self.oracle, self.kind, self.spec = torch, M, oracle, kind, PM.KINDS[kind]
        self.ncrms, self.nx, self.nz, self.T = self.spec["shape"]
        self.dt = PM.DTYPES[self.spec["dtype"]]
        self.exact = variant == "exact"
        M.set_variant(M.VARIANT_EXACT if self.exact else M.VARIANT_FAST)
        if self.spec["ref"]:
            M.set_plan_layout(M.LAYOUT_REFERENCE)
        M.set_tall_columns(int(self.spec["tall"]))
        M.set_f32_odd_ncrms(int(self.spec["odd"]))
        self.model = PM.PlanModel(oracle, self.ncrms, self.nx, self.nz, self.T, self.dt)
        self.shards = PM.shard_ranges(self.ncrms, self.spec["multi"]) if self.spec["multi"] else [(0, self.ncrms)]
        self.p = M.Plan(self.ncrms, self.nx, self.nz, self.T, dtype=self.dt,
                        **({"devices": [0] * self.spec["multi"]} if self.spec["multi"] else {}))
        self.pending, self.alive, self.streams, self.got, self.at = [], [], [], {}, -1

    def check_kind(self):
        M, p, W = self.M, self.p, (w_of(self.nz) if self.spec["tall"] else 1)
        assert p.ngpus == (self.spec["multi"] or 1)
        assert p.level_windows == W and (W >= 5) == bool(self.spec["tall"])
        if self.spec["multi"]:
            assert [(a, n) for _, a, n in p.shards()] == self.shards
            for g in range(p.ngpus):
                sp = p.shard_plan(g)
                assert sp.layout == M.LAYOUT_WAVEMAJOR and sp.level_windows == W and sp.dims[0] == self.shards[g][1]
        else:
            assert p.layout == (M.LAYOUT_REFERENCE if self.spec["ref"] else M.LAYOUT_WAVEMAJOR)

    # ---- comparisons
    def compare(self, i, op, name, got, want, first, bounds):
        """one array of a read-back against the model's (both with a tracer axis); bounds: per tracer (K, S, SF)"""
        what = f"op {i} {op['op']} {name}"
        got = got.reshape(want.shape, order="F")
        assert got.dtype == want.dtype == self.dt
        if self.exact:
            assert_bitwise(got, want, what)
            return
        u, nzm = UNIT[self.dt], self.nz - 1
        for j in range(want.shape[-1]):
            K, S, SF = bounds[first + j]
            g, w = got[..., j].astype(np.float64), want[..., j].astype(np.float64)
            if name == "f":
                d = float(np.max(np.abs(g - w)))
                print(f"{what} tracer {first + j}: max|df| = {d / (u * S):.2f} u S after {K} steps")
                assert d <= K * C_FAST * u * S, f"{what} tracer {first + j}: max|df| = {d:.3e} > {K} * 64 u * {S:.3e}"
            else:
                d = float(np.max(np.abs(g[:, :nzm] - w[:, :nzm])))
                print(f"{what} tracer {first + j}: max|dflux| = {d / (u * SF) if SF else 0:.2f} u S after {K} steps")
                assert d <= K * C_FAST * u * SF, f"{what} tracer {first + j}: max|dflux| = {d:.3e} > {K} * 64 u * {SF:.3e}"
                assert_bitwise(got[:, nzm, j], want[:, nzm, j], what + " level nz")

    def bounds(self):
        m = self.model
        return [(m.steps[t], m.fmax[t], m.flmax[t]) for t in range(self.T)]

    def flush(self):
        """behind a synchronisation of the sequence: the device read-backs since the last one, and the device inputs"""
        for i, op, name, t, want, first, bounds in self.pending:
            got = to_host(t)
            self.got.setdefault(i, {})[name] = got.reshape(want.shape, order="F")
            self.compare(i, op, name, got, want, first, bounds)
        for i, op, name, t, src in self.alive:
            assert_bitwise(to_host(t), src, f"op {i} {op['op']}: the caller's {name} afterwards")
        self.pending, self.alive = [], []

    def dev_in(self, i, op, arrs):
        out = {}
        for k, a in arrs.items():
            a = squeeze(a, k)
            out[k] = to_dev(a)
            self.alive.append((i, op, k, out[k], a))
        return out

    def target(self, i, op, want):
        """{name: device tensor}, NaN pattern, registered for comparison with the model's `want`"""
        out, b = {}, self.bounds()
        for k, w in want.items():
            out[k] = to_dev(squeeze(unwritten(w.shape, self.dt), k))
            self.pending.append((i, op, k, out[k], w, op.get("first", 0), b))
        return out

    def plan_of(self, op):
        """(plan, local sl0) a block op goes to: the shard's own plan on a multi-GPU plan"""
        if not self.spec["multi"] or op["op"] == "handle_block":
            return self.p, op["sl0"]
        return self.p.shard_plan(op["shard"]), op["sl0"] - self.shards[op["shard"]][0]

    # ---- one op on the library; `want` is what the model returned for it
    def do(self, i, op, want):
        M, p, o = self.M, self.p, op["op"]
        if o == "upload":
            a = {k: squeeze(v, k) for k, v in PM.fresh(self.kind, op, self.oracle).items()}
            keep = {k: v.copy(order="F") for k, v in a.items()}
            p.upload(a["f"], a["u"], a["w"], a["rho"], a["rhow"], a["adz"], a["flux"])
            for k in a:
                assert_bitwise(a[k], keep[k], f"op {i} upload: the caller's {k} afterwards")
        elif o == "import_device":
            p.import_device(**self.dev_in(i, op, PM.fresh(self.kind, op, self.oracle)), first_tracer=op["first"])
        elif o == "import_block":
            q, sl0 = self.plan_of(op)
            q.import_block(sl0, **self.dev_in(i, op, PM.fresh(self.kind, op, self.oracle)), first_tracer=op["first"])
        elif o == "run":
            p.run(op.get("first"), op.get("count"))
        elif o == "run_uw":
            d = self.dev_in(i, op, PM.fresh(self.kind, dict(op, names=("u", "w")), self.oracle))
            p.run_uw(d["u"], d["w"], op["first"], op["count"])
        elif o == "set_boundary":
            p.set_boundary(op["mode"])
            assert p.boundary == op["mode"]
        elif o == "export_device":
            p.export_device(**self.target(i, op, want), first_tracer=op["first"])
        elif o in ("export_block", "handle_block"):
            q, sl0 = self.plan_of(op)
            if o == "handle_block":   # refused before any device call: targets of the block's shape, never written
                want = {k: np.zeros((op["n"],) + self.model.a[k].shape[1:-1] + (op["ntr"],), self.dt, order="F") for k in op["what"]}
                q.export_block(sl0, **{k: to_dev(squeeze(v, k)) for k, v in want.items()}, first_tracer=op["first"])
            else:
                q.export_block(sl0, **self.target(i, op, want), first_tracer=op["first"])
        elif o in ("download", "download_block"):
            host = {k: squeeze(unwritten(w.shape, self.dt), k) for k, w in want.items()}
            if o == "download":
                p.download(host["f"], host["flux"])
                self.flush()      # (synchronous: every stream of the plan has drained)
            else:
                q, sl0 = self.plan_of(op)
                q.download_block(sl0, host.get("f"), host.get("flux"))
            b = self.bounds()
            for k, w in want.items():
                self.got.setdefault(i, {})[k] = host[k].reshape(w.shape, order="F")
                self.compare(i, op, k, host[k], w, 0, b)
        elif o == "timing":
            p.set_timing(op["on"])
            ms = p.last_kernel_ms()    # (raises where the model says MPDATA_ESTATE)
            assert ms > 0, f"op {i}: last_kernel_ms = {ms}"
        elif o == "set_stream":
            s = self.torch.cuda.Stream() if op["new"] else self.torch.cuda.default_stream()
            self.streams.append(s)
            p.set_stream(s)
            self.flush()          # (set_stream drains the stream the plan leaves)
        elif o == "sync":
            p.sync()
            self.flush()
        else:
            raise ValueError(o)

    def play(self, ops):
        M = self.M
        for i, op in enumerate(ops):
            self.at = i
            want = PM.apply(self.model, self.kind, op, self.oracle)
            err = want if isinstance(want, int) and not isinstance(want, bool) else None
            assert err == op.get("err"), f"op {i}: the model returned {want!r}, the generator recorded {op.get('err')}"
            assert self.model.finite()
            if err is None:
                self.do(i, op, want)
                continue
            n_pending = len(self.pending)
            with pytest.raises(M.MpdataError) as e:
                self.do(i, op, want)
            assert e.value.code == err, f"op {i} {op['op']}: raised {e.value.code}, the model says {err}"
            del self.pending[n_pending:]
        assert not self.pending and not self.alive
        n = len(ops)
        for k in ("f", "flux"):
            assert_bitwise(self.got[n - 2][k], self.got[n - 1][k], f"final export_device against final download, {k}")


@pytest.mark.parametrize("kind,seed,variant", CASES, ids=[f"{k}-{s}-{v}" for k, s, v in CASES])
def test_sequence(M, oracle, kind, seed, variant):
    ops = PM.sequences(kind, seed, PM.LENGTH, oracle)
    pl = Player(M, oracle, kind, variant)
    try:
        pl.check_kind()
        pl.play(ops)
    except Exception as e:
        raise AssertionError(f"{kind} seed {seed} {variant}: {type(e).__name__} at op {pl.at}: {e}\n"
                             f"ops up to there (PM.apply on a PlanModel, Player.do on a Plan replay them):\n"
                             f"{json.dumps(ops[:pl.at + 1])}\n"
                             f"to run this case alone: pytest tests/test_plan_sequences.py -m gpu -k {kind}-{seed}-{variant}") from e
    finally:
        pl.p.close()
