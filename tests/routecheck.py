"""What the device-route tests share that needs no torch: the runner of the child-process cases (tests/*_torch_cases.py), the error code
of a refused call, and the comparison of a guard-filled buffer with the records expected in it.  Nothing here imports torch, so the pytest
process can import it before the package (whose import decides _TORCH_FIRST)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(module, case, *args, timeout=600):
    """`python tests/<module>.py <case> <args...>` in a child process (torch has to be imported before the package there): it exits 0 and
    has printed "ok <case>"."""
    r = subprocess.run([sys.executable, os.path.join(HERE, module + ".py"), case] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, cwd=HERE)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert ("ok " + case) in r.stdout, r.stdout[-3000:]


def code(rt, fn):
    """the PtError code with which fn() is refused"""
    try:
        fn()
    except rt.PtError as e:
        return e.code
    raise AssertionError("no error")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_guarded(got, want, guard, tag=(), offsets=None):
    """`got`, a (rows, w) uint32 buffer that was filled with `guard` before the query wrote into it, begins with the len(want) records
    `want`, and every row behind them still holds the guard: a store beyond the records, or a record left out, shows.  offsets: the
    (written, expected) offsets of a list query, which are equal whatever the capacity was."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and want.dtype == np.uint32 and len(want) <= len(got), tag
    if offsets is not None:
        assert np.array_equal(offsets[0], offsets[1]), (tag, np.flatnonzero(np.asarray(offsets[0]) != np.asarray(offsets[1]))[:8])
    assert got.ndim == 2 and want.shape == (len(want), got.shape[1]), tag
    held = len(want)
    assert np.array_equal(got[:held], want), (tag, np.flatnonzero((got[:held] != want).any(1))[:8])
    assert np.all(got[held:] == np.uint32(guard)), (tag, np.flatnonzero((got[held:] != np.uint32(guard)).any(1))[:8] + held)
