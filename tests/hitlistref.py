"""Independent statements of what the hit lists hold (include/mi355pt.h pt_list_hits), in numpy:

  * hit_records():  pt_device.h::tri_hit and pt_rayquery.hip::hit_record restated in float32, operation by operation, for every
                    (ray, triangle) pair: crossref.hit_matrix extended to t, u, v
  * brute_lists():  the list of every ray over ALL triangles in index order -- what PT_HITS_BRUTE_FORCE must return, bit for bit
  * sort_lists():   every list into ascending (t bits << 32 | prim)
  * float64_pairs(): Moller-Trumbore in float64 on the f32-rounded e1, e2, with the band in which float32 may decide differently
"""
import numpy as np

from crossref import EPS, INF_T, _cross, _dot, ray_walked

f32 = np.float32


def hit_records(O, D, t_max, tris):
    """(rays, triangles) arrays (ok, t, u, v): tri_hit(o, d, record) and t < min(t_max, 1e30), with the t of the test and the u, v of
    hit_record (the same operations as the test's own); every operation a float32 operation in the order of pt_device.h."""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)
    v0 = [T[None, :, 0, k] for k in range(3)]
    e1 = [(T[:, 1, k] - T[:, 0, k])[None, :] for k in range(3)]      # the record's e1, e2: rounded once at upload
    e2 = [(T[:, 2, k] - T[:, 0, k])[None, :] for k in range(3)]
    o = [np.asarray(O, f32)[:, k, None] for k in range(3)]
    d = [np.asarray(D, f32)[:, k, None] for k in range(3)]
    best = np.minimum(np.asarray(t_max, f32), INF_T)[:, None]
    with np.errstate(all="ignore"):
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        ok = ~(np.abs(det) < EPS)
        inv_det = f32(1.0) / det
        sv = [o[k] - v0[k] for k in range(3)]
        u = inv_det * _dot(sv, pv)
        ok &= ~((u < 0) | (u > 1))
        q = _cross(sv, e1)
        v = inv_det * _dot(d, q)
        ok &= ~((v < 0) | ((u + v) > 1))
        t = inv_det * _dot(e2, q)
        ok &= (t > EPS) & (t < best)
    assert t.dtype == f32 and u.dtype == f32 and v.dtype == f32
    return ok, t, u, v


def brute_lists(rays, tris, cells=4_000_000):
    """(offsets, t, prim, u, v) of PtRay records over all triangles, lists in index order; empty for a ray that is not walked."""
    r = np.asarray(rays, f32).reshape(-1, 8)
    n_tris = np.asarray(tris).size // 9
    counts = np.zeros(len(r), np.int64)
    cols = [[], [], [], []]
    walked = np.flatnonzero(ray_walked(r))
    step = max(1, cells // max(n_tris, 1))
    for a in range(0, len(walked), step):
        i = walked[a:a + step]
        ok, t, u, v = hit_records(r[i, 0:3], r[i, 4:7], r[i, 3], tris)
        counts[i] = ok.sum(axis=1)
        ri, ti = np.nonzero(ok)                                        # row-major: ray by ray, triangles ascending
        for c, x in zip(cols, (t[ri, ti], ti.astype(np.uint32), u[ri, ti], v[ri, ti])):
            c.append(x)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    t, prim, u, v = (np.concatenate(c) if c else np.zeros(0, k) for c, k in zip(cols, (f32, np.uint32, f32, f32)))
    return offsets, t.astype(f32), prim.astype(np.uint32), u.astype(f32), v.astype(f32)


def sort_lists(res):
    """(offsets, t, prim, u, v) with every list in ascending order of the 64-bit key (t bits << 32) | prim (stable)."""
    offsets, t, prim, u, v = res[:5]
    off = np.asarray(offsets).astype(np.int64)
    own = np.repeat(np.arange(len(off) - 1), np.diff(off))
    key = (np.asarray(t, f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(prim, np.uint32).astype(np.uint64)
    order = np.lexsort((key, own))
    return (offsets,) + tuple(np.asarray(a)[order] for a in (t, prim, u, v))


def float64_pairs(rays, tris):
    """Moller-Trumbore in float64 on the f32-rounded e1, e2 for every (ray, triangle) pair of walked rays.  Returns (hit, band, t, u, v),
    each (rays, triangles): `band` marks the pairs float32 may decide differently -- one of |u|, |v|, |1 - u - v| below 1e-4, t within
    1e-4 max(1, t) of t_max or of 1e-7, |det| within 1 % of 1e-7."""
    r = np.asarray(rays, f32).reshape(-1, 8)
    T = np.asarray(tris, f32).reshape(-1, 3, 3)
    v0 = T[None, :, 0].astype(np.float64)
    e1 = (T[:, 1] - T[:, 0]).astype(np.float64)[None]
    e2 = (T[:, 2] - T[:, 0]).astype(np.float64)[None]
    o = r[:, None, 0:3].astype(np.float64); d = r[:, None, 4:7].astype(np.float64)
    best = np.minimum(r[:, 3].astype(np.float64), 1e30)[:, None]
    eps = float(EPS)
    with np.errstate(all="ignore"):
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        inv = 1.0 / det
        sv = o - v0
        u = inv * (sv * pv).sum(-1)
        q = np.cross(sv, e1)
        v = inv * (d * q).sum(-1)
        t = inv * (e2 * q).sum(-1)
        hit = ~(np.abs(det) < eps) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > eps) & (t < best)
        band = (np.abs(u) < 1e-4) | (np.abs(v) < 1e-4) | (np.abs(1 - u - v) < 1e-4)
        band |= (np.abs(t - best) <= 1e-4 * np.maximum(1, np.abs(t))) | (np.abs(t - eps) <= 1e-4 * np.maximum(1, np.abs(t)))
        band |= np.abs(np.abs(det) - eps) <= 0.01 * eps
    return hit, band, t, u, v
