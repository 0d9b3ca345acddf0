"""What the tests of the Fortran test programs (tests/fortran/*_calls.F90) share: the record streams the programs read and
write, one run of a program, the comparison of its dump with a replay, and the records of the frame the six single-call
programs have in common (tests/fortran/calls_common.F90: calls_import in front of the calls under test, calls_close
behind them)."""
import os
import struct
import subprocess

import numpy as np

from oracle import plan_model as PM
from util import assert_bitwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {1: np.int32, 2: np.int64, 3: np.float32, 4: np.float64}
CODE = {np.dtype(v): k for k, v in KIND.items()}


# ------------------------------------------------------------------------------------------------ the record streams
def write_records(path, records, end=False):
    """records: (name, array) -- name (16 characters), kind, rank, dims, the data in Fortran order; end: the closing record
    the program puts behind its dump"""
    with open(path, "wb") as fh:
        for name, a in records:
            a = np.asarray(a)
            assert len(name) <= 16 and name != "end"
            fh.write(name.ljust(16).encode() + struct.pack("<ii", CODE[a.dtype], a.ndim) + struct.pack(f"<{a.ndim}q", *a.shape))
            fh.write(a.tobytes(order="F"))
        if end:
            fh.write(b"end".ljust(16) + struct.pack("<ii", 1, 0))


def read_records(path):
    """-> [(name, array)], up to the program's closing record `end` (a dump without one is cut short)"""
    raw, off, out = open(path, "rb").read(), 0, []
    while True:
        assert off + 24 <= len(raw), f"the dump ends after {len(out)} records without its closing record"
        name = raw[off:off + 16].decode().rstrip()
        kind, rank = struct.unpack_from("<ii", raw, off + 16)
        off += 24
        if name == "end":
            assert off == len(raw)
            return out
        dims = struct.unpack_from(f"<{rank}q", raw, off)
        off += 8 * rank
        dt = np.dtype(KIND[kind])
        cnt = int(np.prod(dims))
        out.append((name, np.frombuffer(raw, dt, cnt, off).reshape(dims, order="F")))
        off += cnt * dt.itemsize


# ------------------------------------------------------------------------------------------------ one run, one comparison
def run_program(exe_name, records, tmp_path):
    """tests/fortran/<exe_name> on an input file of `records`, without MPDATA_* in its environment -> its dump, parsed"""
    exe = os.path.join(ROOT, "tests", "fortran", exe_name)
    assert os.path.exists(exe), f"{exe} is not built (run __graft_entry__.build())"
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    write_records(fin, records)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MPDATA_")}
    res = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return read_records(fout)


def compare_dump(got, want, label):
    """the names of the records in order, then every record bit for bit"""
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        assert_bitwise(a, np.asfortranarray(b).reshape(a.shape, order="F"), f"{label}: record {k}")


# ------------------------------------------------------------------------------------------------ the frame of the six replays
def rc(what, code=None):
    """the record of a call's return code; None, a model call's answer when it accepts, is 0"""
    return ("rc:" + what, np.array([0 if code is None else code], np.int32))


def want_import(m, inp):
    """calls_import on the model m: the PERIODIC plan filled with the seven arrays of inp"""
    return [rc("set_variant"), rc("create"), rc("set_boundary", m.set_boundary(PM.PERIODIC)),
            rc("import", m.import_device({k: np.array(inp[k], order="F") for k in PM.NAMES}))]


def want_close(m):
    """calls_close on the model m: a step and the read-back"""
    run = m.run()
    e = m.export_device()
    return [rc("run", run), rc("sync"), rc("export"), rc("sync"), ("f_e", e["f"]), ("flux_e", e["flux"]), rc("destroy")]
