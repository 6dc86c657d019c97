"""Independent statements of what the crossing queries compute (include/mi355pt.h), in numpy:

  * crossings():      pt_device.h::tri_hit restated in float32, operation by operation, summed over ALL triangles -- what
                      PT_COUNT_BRUTE_FORCE must return, bit for bit in every comparison
  * winding_number(): the generalised winding number of a triangle mesh around a point in float64 (the solid angles of the triangles by
                      Van Oosterom & Strackee's formula, summed, over 4 pi): +-1 inside a closed mesh, 0 outside -- it shares nothing with
                      ray casting
  * reaches():        whether the boxes on the way from the root of a reference-layout BVH4 to a triangle's leaf all pass the slab test of
                      a ray (float32, pt_device.h::slab): names the triangle a walk lost to a box
"""
import numpy as np

f32 = np.float32
EPS = f32(1e-7)
INF_T = f32(1e30)
LEAF, INVALID = 0x80000000, 0xFFFFFFFF


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def hit_matrix(O, D, t_max, tris):
    """(rays, triangles) bool: tri_hit(o, d, record) and t < min(t_max, 1e30); every operation a float32 operation in the order of pt_device.h."""
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
    assert det.dtype == f32 and t.dtype == f32
    return ok


def ray_walked(rays):
    r = np.asarray(rays, f32).reshape(-1, 8)
    return ~np.isnan(r[:, [0, 1, 2, 4, 5, 6]]).any(axis=1) & (r[:, 3] > 0)


def crossings(rays, tris, cells=4_000_000):
    """uint32 per PtRay record: the number of triangles it crosses; 0 for a ray that is not walked."""
    r = np.asarray(rays, f32).reshape(-1, 8)
    n_tris = np.asarray(tris).size // 9
    out = np.zeros(len(r), np.uint32)
    walked = np.flatnonzero(ray_walked(r))
    step = max(1, cells // max(n_tris, 1))
    for a in range(0, len(walked), step):
        i = walked[a:a + step]
        out[i] = hit_matrix(r[i, 0:3], r[i, 4:7], r[i, 3], tris).sum(axis=1)
    return out


def crossed_triangles(ray, tris):
    r = np.asarray(ray, f32).reshape(1, 8)
    return np.flatnonzero(hit_matrix(r[:, 0:3], r[:, 4:7], r[:, 3], tris)[0])


def winding_number(points, tris, chunk=1024):
    """float64 generalised winding number of the mesh around each point."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    out = np.zeros(len(P))
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        a, b, c = T[None, :, 0] - p, T[None, :, 1] - p, T[None, :, 2] - p
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = np.einsum("ijk,ijk->ij", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ijk,ijk->ij", a, b) * lc + np.einsum("ijk,ijk->ij", b, c) * la + np.einsum("ijk,ijk->ij", c, a) * lb
        out[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def _halves(w):
    return np.array([w & 0xFFFF, w >> 16], np.uint16).view(np.float16).astype(f32)


def slab(o, d, box, best):
    """pt_device.h::slab of one packed f16 box in float32 -> (passes, tmin)."""
    with np.errstate(all="ignore"):
        inv = np.where(np.abs(d) > f32(1e-8), f32(1.0) / d, INF_T).astype(f32)
        h0, h1, h2 = _halves(int(box[0])), _halves(int(box[1])), _halves(int(box[2]))
        mn = np.array([h0[0], h0[1], h1[0]], f32); mx = np.array([h1[1], h2[0], h2[1]], f32)
        t1 = (mn - o) * inv; t2 = (mx - o) * inv
        tmin = np.fmax(np.fmax(np.fmin(t1[0], t2[0]), np.fmin(t1[1], t2[1])), np.fmin(t1[2], t2[2]))
        tmax = np.fmin(np.fmin(np.fmax(t1[0], t2[0]), np.fmax(t1[1], t2[1])), np.fmax(t1[2], t2[2]))
    return bool(tmax >= np.fmax(tmin, f32(0))) and bool(tmin < best), tmin


def reaches(bvh4, ray, tri):
    """Whether every box from the root down to the leaf of triangle `tri` passes the ray's slab test; the first node that fails otherwise."""
    b = np.asarray(bvh4, np.uint32)
    m = int(b[0]); rec = b[1:1 + 8 * m].reshape(m, 8)
    parent = np.full(m, -1, np.int64)
    for i in np.flatnonzero((rec[:, 7] & LEAF) == 0):
        for c in rec[i, 3:7]:
            if c != INVALID and c < m:
                parent[int(c)] = i
    leaves = np.flatnonzero(((rec[:, 7] & LEAF) != 0) & ((rec[:, 7] & 0x7FFFFFFF) == tri))
    r = np.asarray(ray, f32).reshape(8)
    best = min(r[3], INF_T)
    for node in leaves:
        chain = []
        while node >= 0:
            chain.append(int(node)); node = parent[node]
        if chain[-1] != 0:
            continue
        for i in reversed(chain):
            if not slab(r[0:3], r[4:7], rec[i, 0:3], best)[0]:
                return False, i
        return True, None
    return False, None
