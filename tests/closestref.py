"""An independent float64 statement of "which triangle is nearest to this point", in numpy, for the closest-point tests.

Written differently from the product (pt_closest.h: a Gram-Schmidt step and Eberly's regions on (p - v0, e1, e2) in f32): here a point is projected onto
the triangle's plane; if the projection lies inside, it is the closest point; otherwise the closest point is the nearest of the three
closest points on the edge segments.  Every triangle is considered for every point: the triangles are processed in chunks, a chunk's
squared centroid distances come from one matrix product, and a triangle is evaluated exactly unless its bounding sphere proves it farther
than a triangle whose exact distance is already known (|p - c| - r > upper bound, with a margin far above the rounding of the product)."""
import numpy as np

f64 = np.float64


def _segment(p, a, b):
    ab = b - a
    den = np.einsum("ij,ij->i", ab, ab)
    t = np.einsum("ij,ij->i", p - a, ab) / np.where(den > 0, den, 1.0)
    t = np.clip(np.where(den > 0, t, 0.0), 0.0, 1.0)
    return a + ab * t[:, None]


def closest_on_triangles(p, tri):
    """Pairwise: p (k, 3) f64, tri (k, 3, 3) f64 -> (distance (k,), closest point (k, 3))."""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    n = np.cross(b - a, c - a)
    nn = np.einsum("ij,ij->i", n, n)
    flat = nn > 0
    safe = np.where(flat, nn, 1.0)
    q = p - n * (np.einsum("ij,ij->i", p - a, n) / safe)[:, None]           # the projection onto the plane
    # inside iff the three sub-triangle normals point along n
    s0 = np.einsum("ij,ij->i", np.cross(b - a, q - a), n)
    s1 = np.einsum("ij,ij->i", np.cross(c - b, q - b), n)
    s2 = np.einsum("ij,ij->i", np.cross(a - c, q - c), n)
    inside = flat & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    best = np.where(inside[:, None], q, 0.0)
    d = np.where(inside, np.linalg.norm(p - q, axis=1), np.inf)
    for u, v in ((a, b), (b, c), (c, a)):
        e = _segment(p, u, v)
        de = np.linalg.norm(p - e, axis=1)
        take = ~inside & (de < d)
        best = np.where(take[:, None], e, best); d = np.where(take, de, d)
    return d, best


def distance_to(points, tris, prim):
    """f64 distance from points[i] to triangle prim[i]."""
    t = np.asarray(tris, f64).reshape(-1, 3, 3)[np.asarray(prim, np.int64)]
    return closest_on_triangles(np.asarray(points, f64).reshape(-1, 3), t)[0]


def nearest(points, tris, chunk=2048, mask=None):
    """For every point the f64 minimum distance over ALL triangles (mask: bool per triangle, False = left out) and one triangle at it.
    Returns (dist (n,), prim (n,))."""
    p = np.asarray(points, f64).reshape(-1, 3)
    t = np.asarray(tris, f64).reshape(-1, 3, 3)
    ids = np.arange(t.shape[0]) if mask is None else np.nonzero(mask)[0]
    t = t[ids]
    n, m = p.shape[0], t.shape[0]
    if m == 0:
        return np.full(n, np.inf), np.full(n, -1, np.int64)
    cen = t.mean(1)
    rad = np.linalg.norm(t - cen[:, None, :], axis=2).max(1)
    pa = np.concatenate([p, np.einsum("ij,ij->i", p, p)[:, None], np.ones((n, 1))], 1)              # [p, |p|^2, 1]
    ca = np.concatenate([-2.0 * cen, np.ones((m, 1)), np.einsum("ij,ij->i", cen, cen)[:, None]], 1)  # [-2c, 1, |c|^2]
    scale = 1.0 + float(np.abs(p).max(initial=0.0)) ** 2 + float(np.abs(cen).max()) ** 2
    # sweep 1: the triangle with the nearest centroid gives an upper bound (its exact distance)
    cbest = np.full(n, np.inf); cidx = np.zeros(n, np.int64)
    for s in range(0, m, chunk):
        d2 = pa @ ca[s:s + chunk].T
        k = d2.argmin(1); v = d2[np.arange(n), k]
        take = v < cbest
        cbest = np.where(take, v, cbest); cidx = np.where(take, k + s, cidx)
    best, _ = closest_on_triangles(p, t[cidx])
    prim = cidx.copy()
    # sweep 2: every triangle whose sphere does not prove it farther than the bound is evaluated exactly
    for s in range(0, m, chunk):
        d2 = pa @ ca[s:s + chunk].T
        reach = best + rad[s:s + chunk].max()
        pi, ti = np.nonzero(d2 <= (reach * reach + 1e-9 * scale)[:, None])
        if pi.size == 0:
            continue
        d, _ = closest_on_triangles(p[pi], t[ti + s])
        order = np.lexsort((ti, d, pi))                     # per point: the smallest distance first
        pi, ti, d = pi[order], ti[order], d[order]
        first = np.concatenate([[True], pi[1:] != pi[:-1]])
        pi, ti, d = pi[first], ti[first], d[first]
        take = d < best[pi]
        best[pi[take]] = d[take]; prim[pi[take]] = ti[take] + s
    return best, ids[prim]
