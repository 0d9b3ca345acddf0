"""CPU test of the column-group geometry the five LDS-staging block kernels are launched with (csrc/mpdata_wm_walk.h:
col_groups_batched for column_path, vsolve and column_step, col_groups_tiled for sediment and cell_add).  A stand-alone
host program (tests/stubs/col_groups_probe.cpp, its own main, no device) calls the two entry points with the arguments
the launchers pass, over the table of tests/col_groups_cases.py: every (slp, nlev) mpdata_plan_create produces for
nz = 2 .. 238 and the inner plans of windowed nz = 239, 250, 300, 1000, both precisions (fp32 plans odd: a phantom), nine
nx, six blocks each, cell-add without and with dsum, and refused jobs for the guards.  Every field and every
accept / refuse decision is compared with tests/golden/col_groups_parent.npz, which was recorded from the launchers'
own arithmetic before it was shared (docs/EXPERIMENTS.md Z): the kernels are launched as they were.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import col_groups_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "codesign-kernels_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "col_groups_parent.npz")


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    hipcc = shutil.which("hipcc")
    if hipcc:
        inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
        if os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
            return inc
    return None


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx, inc = shutil.which("g++"), _rocm_include()
    if not cxx or not inc:
        pytest.skip("no g++ or no HIP headers here")
    exe = str(tmp_path_factory.mktemp("col_groups") / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC,
                    os.path.join(HERE, "stubs", "col_groups_probe.cpp"), "-o", exe], check=True)
    return exe


def test_table_is_the_recorded_one():
    want = np.load(GOLDEN)["table"].T
    got = np.array(C.cases(), dtype=np.int64)
    assert got.shape == want.shape and np.array_equal(got, want)
    # what the table must hold
    plans = {(c[8], c[1]) for c in C.plan_cases()}
    assert plans == {(nz, ipe) for nz in list(range(2, 239)) + [239, 250, 300, 1000] for ipe in (1, 2)}
    per_plan = {}
    for c in C.plan_cases():
        per_plan.setdefault((c[8], c[1]), set()).add((c[0], c[4], c[9], c[10]))
    for (nz, ipe), s in per_plan.items():
        calls = 6 if nz <= 238 else 5
        assert len(s) == calls * len(C.NX) * 6, (nz, ipe)
        assert {x[1] for x in s} == set(C.NX)


def test_geometry_is_the_parents(probe):
    z = np.load(GOLDEN)
    cases = C.cases()
    txt = "".join(C.line(c) + "\n" for c in cases)
    out = subprocess.run([probe], input=txt, capture_output=True, text=True, check=True).stdout
    got = np.array(C.parse(out), dtype=np.int64)
    want = z["result"].T
    assert got.shape == want.shape == (len(cases), 1 + len(C.FIELDS))      # no case is left out
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, [(C.line(cases[i]), want[i].tolist(), got[i].tolist()) for i in bad[:5]]
    # the fixture itself: every plan's job is accepted, and every guard that can be reached refuses something
    nplan = sum(1 for _ in C.plan_cases())
    assert want[:nplan, 0].all()
    guards = want[nplan:]
    assert (guards[:, 0] == 0).sum() >= 30
    # column_path counts units in long long: it runs the plan of 2^31 units the int kernels refuse
    beyond = [i for i, c in enumerate(cases) if c[6] == (1 << 31) + 8]
    assert [int(want[i, 0]) for i in beyond] == [1, 0, 0, 0, 0, 0]
