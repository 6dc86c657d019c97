"""Scenes, bounds and kernel-style shadow-ray origins shared by tests/test_exposure_reference.py (CPU) and tests/test_gpu_exposure.py."""
import functools

import numpy as np

import exposeref
from scenes import random_soup

LZ = 1.0 / np.sqrt(4.25)          # the light's z component (x the same, y 1.5 times it)
CAM = 4.0                         # ray origins of the tests lie within this distance of the origin
GATE32 = np.float32(0.1002)       # pt_device.h::kExposeGate


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def _grid(nx, ny, x0, x1, y0, y1, z):
    t = []
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    for i in range(nx):
        for j in range(ny):
            t += _quad((xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z))
    return t


def torus(nu=40, nv=24, big=1.0, small=0.4, bump=0.03):
    def p(i, j):
        u, v = 2 * np.pi * (i % nu) / nu, 2 * np.pi * (j % nv) / nv
        r = small * (1.0 + bump * np.sin(5 * u) * np.cos(3 * v))
        return ((big + r * np.cos(v)) * np.cos(u), (big + r * np.cos(v)) * np.sin(u), r * np.sin(v))
    t = []
    for i in range(nu):
        for j in range(nv):
            t += _quad(p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1))
    return np.array(t, np.float32)


def plates():
    return np.array(_grid(8, 8, -1, 1, -1, 1, 0.0) + _grid(4, 4, -0.9, 0.1, -0.9, 0.1, 0.5), np.float32)


def vfold(delta, lean=1.5):
    """A floor [0,1]^2 at z = 0 and a wing whose lower edge hovers 3e-4 over the floor's edge x = 1 and whose shadow on the plane z = 0 reaches `delta` into the
    floor there (delta < 0: a gap; the shadow-ray origins lie 1e-4 higher, so they are reached from delta = 1e-4 on); the wing rises to z = 1 leaning by `lean` in x: beyond the light's slope (1) its shadow falls away from the
    floor, below it over the floor."""
    z0 = 3e-4
    xb = 1.0 - delta + z0
    wing = _quad((xb, -1.0, z0), (xb, 2.5, z0), (xb + lean, 2.5, 1.0), (xb + lean, -1.0, 1.0))
    return np.array(_grid(4, 4, 0, 1, 0, 1, 0.0) + wing, np.float32)


def edge_on_wall():
    """a floor and a wall whose plane contains the light direction (its normal is across the light)"""
    wall = _quad((0.3, 0.2, 0.01), (0.3 + 0.2, 0.2 + 0.3, 0.21), (0.3 + 0.2, 0.2 + 0.3, 0.41), (0.3, 0.2, 0.21))
    return np.array(_grid(6, 6, 0, 1, 0, 1, 0.0) + wall, np.float32)


def slivers():
    """a floor under small triangles whose |det| for the light lies around 1e-7 (pt_device.h::kTriEps)"""
    t = _grid(6, 6, 0, 1, 0, 1, 0.0)
    for k, a in enumerate(np.linspace(1.2e-4, 3.2e-4, 21)):
        x, y = 0.1 + 0.04 * k, 0.5
        t.append([(x, y, 0.01), (x + 1e-3, y, 0.01), (x, y + a, 0.01)])
    return np.array(t, np.float32)


def duplicate():
    t = _grid(4, 4, 0, 1, 0, 1, 0.0)
    return np.array(t + [t[5], t[5]], np.float32)


SCENES = {
    "torus": torus, "soup": lambda: random_soup(300, 11).reshape(-1, 3, 3), "plates": plates,
    "vfold_free": lambda: vfold(-0.05), "vfold_over": lambda: vfold(0.3, lean=0.2), "vfold_lip": lambda: vfold(1.5e-4),
    "edge_on": edge_on_wall, "slivers": slivers, "duplicate": duplicate,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    t = np.ascontiguousarray(SCENES[name](), np.float32).reshape(-1, 3, 3)
    t.setflags(write=False)
    return t


def bounds(tris, cam=CAM):
    """(s_max, d_max) of pt_expose.h::Bounds for ray origins within `cam` of the origin"""
    r = float(np.linalg.norm(np.asarray(tris, np.float64).reshape(-1, 3), axis=1).max()) + 1e-3
    return max(cam, r) + r + 1e-3, r + 1e-3


def dot32(a, b):
    return np.float32(np.float32(np.float32(a[0] * b[0]) + np.float32(a[1] * b[1])) + np.float32(a[2] * b[2]))


def aimed_rays(tris, which, per_tri, seed):
    """rays towards points of the triangles `which`: inside, near the edges and near the corners (offsets from 1e-6 of an edge up), from
    both sides, from origins within CAM of the origin; unit directions in f32"""
    rng = np.random.default_rng(seed)
    t = np.asarray(tris, np.float64)
    out = []
    for k in which:
        a, b, c = t[k]
        for s in range(per_tri):
            kind = s % 4
            u, v = rng.random(2)
            if u + v > 1:
                u, v = 1 - u, 1 - v
            if kind == 1:
                v = 10.0 ** rng.uniform(-6, -2)                   # near the edge a-b
            elif kind == 2:
                u = 1.0 - v - 10.0 ** rng.uniform(-6, -2)          # near the edge b-c
            elif kind == 3:
                u, v = 10.0 ** rng.uniform(-6, -2), 10.0 ** rng.uniform(-6, -2)      # near the corner a
            p = a + u * (b - a) + v * (c - a)
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            o = p - d * rng.uniform(0.05, 2.0)
            if np.linalg.norm(o) > CAM:
                continue
            o32 = o.astype(np.float32)
            d32 = (p - o32.astype(np.float64)); d32 = (d32 / np.linalg.norm(d32)).astype(np.float32)
            out.append((o32, d32))
    return out


def shadow_origin(o, d, t, n32):
    """the kernel's shadow-ray origin for a hit at parameter t of a triangle with stored normal n32, or None when the kernel traces the ray
    anyway (the light behind the hit side, or a hit below the gate): pt_megakernel_loop.inc, f32 operation for operation"""
    t = np.float32(t)
    nd = dot32(n32, d)
    nf = n32 if nd < 0 else -n32
    hp = (o + (d * t).astype(np.float32)).astype(np.float32)
    so = (hp + (nf * np.float32(1e-4)).astype(np.float32)).astype(np.float32)
    if not (dot32(nf, exposeref.light32()) > 0) or not (abs(nd) >= GATE32):
        return None
    return so
