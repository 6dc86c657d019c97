"""The two exposure tiers in the tests: the gates, a scene that separates them, and the reference of
tests/exposeref.py evaluated at a gate of the caller's choice -- exposeref.GATE and exposure_cases.GATE32 are set for the time of a call and
put back -- and cached, so that the CPU and the GPU tests of one run share it."""
import contextlib
import functools

import numpy as np

import exposeref
import exposure_cases as xc

GATES = {1: (0.0999, np.float32(0.1002)), 2: (0.2999, np.float32(0.3008))}      # tier: (pt_expose.h f64 gate, pt_device.h f32 gate)
SLACK = 1e-11                                                                   # the band of tests/test_exposure_reference.py


@contextlib.contextmanager
def tier(k):
    old = exposeref.GATE, xc.GATE32
    exposeref.GATE, xc.GATE32 = GATES[k]
    try:
        yield
    finally:
        exposeref.GATE, xc.GATE32 = old


def bumpy_plate():
    """36 x 36 quads over [-0.135, 0.135]^2 whose heights are bilinear over a lattice of every second grid line with values of +-3.5e-3: edges
    of 7.5e-3 and bumps of the same size, so that a concave neighbour lies within the first tier's in-plane margin of most triangles and
    outside the second's.  2,592 triangles."""
    lat = (np.random.default_rng(3).random((20, 20)) - 0.5) * 7e-3
    xs = np.linspace(-0.135, 0.135, 37)

    def p(i, j):
        a, b = i // 2, j // 2
        fa, fb = (i % 2) * 0.5, (j % 2) * 0.5
        z = (1 - fa) * (1 - fb) * lat[a, b] + fa * (1 - fb) * lat[a + 1, b] + (1 - fa) * fb * lat[a, b + 1] + fa * fb * lat[a + 1, b + 1]
        return (xs[i], xs[j], z)
    t = []
    for i in range(36):
        for j in range(36):
            t += xc._quad(p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1))
    return np.array(t, np.float32)


NAMES = sorted(xc.SCENES) + ["bumpy_plate"]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name != "bumpy_plate":
        return xc.scene(name)
    t = np.ascontiguousarray(bumpy_plate(), np.float32).reshape(-1, 3, 3)
    t.setflags(write=False)
    return t


_flags = {}


def flags(tris, k, s_max, d_max, slack=0.0, key=None, **kw):
    """exposeref.flags at tier k's gate; cached under `key` (a scene's name) when one is given"""
    at = None if key is None or kw else (key, k, float(s_max), float(d_max), slack)
    if at is None or at not in _flags:
        with tier(k):
            f = exposeref.flags(tris, s_max, d_max, slack=slack, **kw)
        if at is None:
            return f
        f.setflags(write=False)
        _flags[at] = f
    return _flags[at]


def band(tris, k, s_max, d_max, key=None):
    """(inner, outer): what a mask of tier k has to hold at least and may hold at most"""
    return flags(tris, k, s_max, d_max, SLACK, key), flags(tris, k, s_max, d_max, -SLACK, key)
