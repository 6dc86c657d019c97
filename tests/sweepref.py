"""A float64 brute-force restatement of the sphere-cast query (include/mi355pt.h pt_sweep_spheres): for every sweep
the first t >= 0 at which the centre o + t d lies within r of a triangle, over every triangle -- the overlap at the start, then the face, the
three edges and the three vertices of each triangle with the textbook formulas, none of the product's evaluation order, clamps or box tests.
t_ref(r) is monotone: a larger r never gives a later contact (the set of centres within r of a triangle only grows)."""
import numpy as np

import closestref

f64 = np.float64


def _dot(a, b):
    return (a * b).sum(-1)


def _smaller_root(A, B, C):
    """the smaller root of A t^2 + 2 B t + C = 0 where it exists and is >= 0, else +inf"""
    with np.errstate(all="ignore"):
        disc = B * B - A * C
        t = (-B - np.sqrt(disc)) / A
    return np.where((disc >= 0) & (A > 0) & (t >= 0), t, np.inf)


def pair_times(o, d, r, tri):
    """o, d: (k, 3); r: (k,); tri: (k, 3, 3), all f64 -> (k,) first contact time of each pair, +inf when there is none."""
    v0, v1, v2 = tri[:, 0], tri[:, 1], tri[:, 2]
    dist0, _ = closestref.closest_on_triangles(o, tri)
    out = np.full(len(o), np.inf)
    # face: the plane moved by r towards the side o is on, the touched point inside the triangle
    e1, e2 = v1 - v0, v2 - v0
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n, axis=1)
    with np.errstate(all="ignore"):
        nh = n / ln[:, None]
        h = _dot(nh, o - v0)
        nd = _dot(nh, d)
        t = (np.where(h >= 0, r, -r) - h) / nd
        p = o + d * t[:, None] - nh * np.where(h >= 0, r, -r)[:, None]
        w = p - v0
        a, b, c, d1, d2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(e1, w), _dot(e2, w)
        det = a * c - b * b
        u, v = (c * d1 - b * d2) / det, (a * d2 - b * d1) / det
    ok = (ln > 0) & (t >= 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    out = np.where(ok, np.minimum(out, np.where(ok, t, np.inf)), out)
    # edges: infinite cylinders, the foot of the contact on the segment
    dd = _dot(d, d)
    for a0, a1 in ((v0, v1), (v0, v2), (v1, v2)):
        e = a1 - a0; m = o - a0
        ee = _dot(e, e)
        with np.errstate(all="ignore"):
            md, me, de = _dot(m, d), _dot(m, e), _dot(d, e)
            t = _smaller_root(dd - de * de / ee, md - me * de / ee, _dot(m, m) - me * me / ee - r * r)
            lam = (me + t * de) / ee
        ok = (ee > 0) & np.isfinite(t) & (lam >= 0) & (lam <= 1)
        out = np.minimum(out, np.where(ok, t, np.inf))
    # vertices: spheres
    for a0 in (v0, v1, v2):
        m = o - a0
        out = np.minimum(out, _smaller_root(dd, _dot(m, d), _dot(m, m) - r * r))
    return np.where(dist0 <= r, 0.0, out)


def t_ref(sweeps, tris, radius=None, budget=1 << 18):
    """sweeps: (n, 8) records (org, t_max, dir, radius); radius: (n,) f64 to use in place of the records' -> (t (n,) f64, +inf on a miss;
    prim (n,) int64, -1 on a miss).  Every triangle for every sweep, in chunks of `budget` pairs.  A contact counts only at t < t_max."""
    S = np.asarray(sweeps, f64).reshape(-1, 8)
    T = np.asarray(tris, np.float32).reshape(-1, 3, 3).astype(f64)
    r = S[:, 7] if radius is None else np.asarray(radius, f64)
    n, m = len(S), len(T)
    t = np.full(n, np.inf); prim = np.full(n, -1, np.int64)
    step = max(1, budget // max(m, 1))
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step); k = i1 - i0
        o = np.repeat(S[i0:i1, 0:3], m, axis=0); d = np.repeat(S[i0:i1, 4:7], m, axis=0); rr = np.repeat(r[i0:i1], m)
        tt = pair_times(o, d, rr, np.tile(T, (k, 1, 1))).reshape(k, m)
        j = tt.argmin(axis=1); best = tt[np.arange(k), j]
        hit = best < S[i0:i1, 3]
        t[i0:i1] = np.where(hit, best, np.inf); prim[i0:i1] = np.where(hit, j, -1)
    return t, prim
