"""The plan model and the sequence generator of oracle/plan_model.py, tested on their own (no GPU), so that a failure
of tests/test_plan_sequences.py points at the library: the model's runs against the oracle loop the GPU suites use,
block imports against NumPy slicing, and, for every (kind, seed) the GPU file plays, that the sequence is reproducible,
holds every op class, an expected MPDATA_ESTATE and two steps behind the last import of f, reaches the block edges
its shape allows, and keeps the model finite and f non-zero."""
import numpy as np
import pytest

from oracle import plan_model as PM
from test_plan_tall_columns import make, oracle_steps
from util import assert_bitwise

CASES = [(k, s) for k in PM.KINDS for s in PM.SEEDS[k]]


def filled(oracle, shape, T, dtype, seed=100):
    inp = make(oracle, shape, T=T, dtype=dtype, seed=seed)
    m = PM.PlanModel(oracle, *shape, T, dtype)
    assert m.run() == PM.ESTATE and m.download() == PM.ESTATE and m.last_kernel_ms() == PM.ESTATE
    assert m.import_block(0, 1, {"rho": inp["rho"][:1]}) == PM.ESTATE   # a plan is not first filled block by block
    assert m.upload(inp) is None
    return inp, m


def whole(m, T):
    r = m.download()
    return (r["f"], r["flux"]) if T > 1 else (r["f"][..., 0], r["flux"][..., 0])


@pytest.mark.parametrize("periodic", [False, True], ids=["given", "periodic"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape,T", [((5, 6, 28), 1), ((3, 4, 12), 3)])
def test_model_runs_are_the_oracle_loop(oracle, shape, T, dtype, periodic):
    inp, m = filled(oracle, shape, T, dtype)
    if periodic:
        m.set_boundary(PM.PERIODIC)
    for K in (1, 2, 3):
        assert m.run() is None
        f, flux = whole(m, T)
        f_ref, flux_ref = oracle_steps(oracle, inp, K, periodic=periodic)
        assert_bitwise(f, f_ref, f"{K} runs f")
        assert_bitwise(flux, flux_ref, f"{K} runs flux")
    assert m.steps == [3] * T and m.last_kernel_ms() is True


def test_block_import_is_numpy_slicing(oracle):
    shape, T = (7, 5, 9), 2
    inp, m = filled(oracle, shape, T, np.float64)
    blk = make(oracle, (3,) + shape[1:], T=T, seed=555)
    assert m.import_block(2, 3, {k: blk[k] for k in ("f", "u", "adz", "flux")}) is None
    assert m.import_block(6, 1, {"f": blk["f"][:1, ..., 1:]}, first=1, ntr=1) is None
    want = {k: inp[k].copy(order="F") for k in inp}
    for k in ("f", "u", "adz", "flux"):
        want[k][2:5] = blk[k]
    want["f"][6:7, ..., 1] = blk["f"][:1, ..., 1]
    f, flux = whole(m, T)
    assert_bitwise(f, want["f"], "f")
    assert_bitwise(flux, want["flux"], "flux")
    for k in ("u", "w", "rho", "rhow", "adz"):
        assert_bitwise(m.a[k], want[k], k)
    r = m.export_block(1, 4, ("f",), 1, 1)
    assert set(r) == {"f"}
    assert_bitwise(r["f"][..., 0], want["f"][1:5, ..., 1], "export_block")
    assert m.import_block(5, 3, {"rho": blk["rho"]}) == PM.EINVAL


@pytest.mark.parametrize("periodic", [False, True], ids=["given", "periodic"])
def test_two_tracer_ranges_are_two_whole_steps(oracle, periodic):
    shape, T = (3, 5, 16), 3
    inp, m = filled(oracle, shape, T, np.float64)
    if periodic:
        m.set_boundary(PM.PERIODIC)
    assert m.run() is None and m.run(1, T - 1) is None and m.run(0, 1) is None
    f, flux = whole(m, T)
    f_ref, flux_ref = oracle_steps(oracle, inp, 2, periodic=periodic)
    assert_bitwise(f, f_ref, "f")
    assert_bitwise(flux, flux_ref, "flux")


def test_velocity_and_timing_state(oracle):
    shape, T = (4, 5, 9), 2
    inp, m = filled(oracle, shape, T, np.float64)
    other = make(oracle, shape, seed=977)
    before = whole(m, T)
    assert m.run_uw(other["u"], other["w"], 1, 1) is None and m.steps == [0, 1]
    assert_bitwise(whole(m, T)[0][..., 0], before[0][..., 0], "tracer 0 is not in the range")
    assert m.run() == PM.ESTATE
    assert m.import_block(0, 2, {"u": inp["u"][:2]}) == PM.ESTATE
    assert m.import_device({"u": inp["u"]}) is None                      # u alone: u is held, w is not
    assert m.run() == PM.ESTATE
    assert m.import_block(0, 2, {"u": inp["u"][:2]}) is None
    assert m.import_block(0, 2, {"w": inp["w"][:2]}) == PM.ESTATE
    assert m.import_device({"w": inp["w"]}) is None
    assert m.run() is None and m.steps == [1, 2]
    # set_timing(0): last_kernel_ms is a state error from then on, until a run was recorded with the pair on
    assert m.last_kernel_ms() is True
    m.set_timing(0)
    assert m.last_kernel_ms() == PM.ESTATE
    assert m.run() is None and m.last_kernel_ms() == PM.ESTATE
    m.set_timing(1)
    assert m.last_kernel_ms() == PM.ESTATE
    assert m.run() is None and m.last_kernel_ms() is True
    # PERIODIC -> GIVEN wraps first: the halos are then state
    m.set_boundary(PM.PERIODIC)
    f_p = whole(m, T)[0]
    m.set_boundary(PM.GIVEN)
    assert_bitwise(whole(m, T)[0], f_p, "f after the switch back")
    assert_bitwise(PM.wrap(f_p.copy(order="F")), f_p, "wrap is idempotent")


def is_step(op):
    return op["op"] in ("run", "run_uw") and "err" not in op


@pytest.mark.parametrize("kind,seed", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_sequence_is_reproducible_and_complete(oracle, kind, seed):
    ops = PM.sequences(kind, seed, PM.LENGTH, oracle)
    assert ops == PM.sequences(kind, seed, PM.LENGTH, oracle), "not reproducible"
    spec = PM.KINDS[kind]
    ncrms, nx, nz, T = spec["shape"]
    assert len(ops) == 1 + PM.LENGTH + 3
    assert ops[0]["op"] in ("upload", "import_device") and ops[0]["names"] == list(PM.NAMES) and ops[0]["ntr"] == T
    assert [o["op"] for o in ops[-3:]] == ["sync", "export_device", "download"]
    assert ops[-2]["first"] == 0 and ops[-2]["ntr"] == T and ops[-2]["what"] == ["f", "flux"]
    body = ops[1:-3]
    have = {o["op"] for o in body} | ({"run_sub"} if any(o["op"] == "run" and "first" in o for o in body) else set())
    need = {"import_device", "import_block", "run_sub", "run_uw", "set_boundary", "export_device", "export_block",
            "download", "download_block"} | ({"handle_block"} if spec["multi"] else set())
    assert need <= have, f"missing op classes {need - have}"
    assert any(o.get("err") == PM.ESTATE for o in ops), "no expected MPDATA_ESTATE"
    assert all(o["err"] in (PM.ESTATE, PM.EUNSUPPORTED) for o in ops if "err" in o)
    last_f = max(i for i, o in enumerate(ops) if o["op"] in ("upload", "import_device", "import_block") and "f" in o["names"]
                 and "err" not in o)
    assert sum(is_step(o) for o in ops[last_f + 1:]) >= 2, "fewer than two steps behind the last import of f"
    # the block edges the shape allows (per shard of a multi-GPU plan: shard-local ranges)
    shards = PM.shard_ranges(ncrms, spec["multi"]) if spec["multi"] else [(0, ncrms)]
    blocks = [(o["sl0"] - shards[o["shard"]][0], o["n"], shards[o["shard"]][1]) for o in body if "sl0" in o]
    for o, (a, n, m) in zip([o for o in body if "sl0" in o], blocks):
        assert 0 <= a and 1 <= n and a + n <= m, o
    mmax = max(m for _, m in shards)
    assert any(o["sl0"] + o["n"] == ncrms for o in body if "sl0" in o), "no block ends on the plan's last instance"
    assert any(n == 1 for _, n, _ in blocks), "no block of one instance"
    if mmax >= 2:
        assert any(a % 2 == 1 for a, _, _ in blocks), "no block with an odd sl0"
    if mmax >= 3:
        assert any(a % 2 == 1 and (a + n) % 2 == 1 for a, n, _ in blocks), "no block that splits a pair at both ends"
    # replay on a fresh model: the recorded errors, the step cap, finite, f mostly non-zero
    m = PM.PlanModel(oracle, ncrms, nx, nz, T, PM.DTYPES[spec["dtype"]])
    for i, o in enumerate(ops):
        r = PM.apply(m, kind, o, oracle)
        assert (r if isinstance(r, int) and not isinstance(r, bool) else None) == o.get("err"), (i, o, r)
        assert m.finite(), (i, o)
    assert max(m.steps) <= PM.MAX_STEPS and min(m.steps) >= 1
    assert np.count_nonzero(m.a["f"]) > 0.8 * m.a["f"].size


def test_kinds_cover_the_table():
    """three seeds per kind, every shape of the issue's table once"""
    assert all(len(set(PM.SEEDS[k])) == 3 for k in PM.KINDS) and set(PM.SEEDS) == set(PM.KINDS)
    shapes = sorted((v["shape"], v["dtype"], v["tall"], v["odd"], v["multi"], v["ref"]) for v in PM.KINDS.values())
    assert len(set(shapes)) == len(PM.KINDS) == 22
    assert PM.shard_ranges(7, 2) == [(0, 4), (4, 3)] and PM.shard_ranges(8, 3) == [(0, 3), (3, 3), (6, 2)]
