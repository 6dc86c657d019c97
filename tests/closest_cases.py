"""Shared by the closest-point tests (tests/test_closest_points_host.py, tests/test_gpu_closest_points.py, tests/closest_torch_cases.py):
the point sets, the tolerance against the float64 reference (tests/closestref.py), the set of triangles a tree can reach, and the checks."""
import numpy as np

import closestref

LEAF = 0x80000000
INVALID = 0xFFFFFFFF
MISS = 0xFFFFFFFF
f32 = np.float32

# |twin - float64| <= TOL_K * 2^-24 * (max|p| + max|vertex|).  Measured on the CPU over the point sets of test_closest_points_host.py (every
# scene, every tree, the brute-force route included): the largest deviation of the twin's dist, of the float64 distance of its prim and of
# its (u, v) point from the float64 minimum was MEASURED_K units of 2^-24 * (max|p| + max|vertex|); TOL_K is four times that, rounded up to
# a power of two (the factor covers the difference in evaluation order between point sets).  DESIGN.md section 15 repeats both numbers.
MEASURED_K = 2.60          # dragon50k after the refit; every other scene between 2.14 and 2.41
TOL_K = 16.0


def tolerance(points, tris):
    return TOL_K * 2.0 ** -24 * (float(np.abs(points[:, :3]).max()) + float(np.abs(tris).max()))


def query_points(tris, n, seed):
    """A quarter each: uniform in 1.5x the scene box, on the surface, within 1e-3 of it, far away (+-8)."""
    rng = np.random.default_rng(seed)
    T = np.asarray(tris, f32).reshape(-1, 3, 3)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    mid, half = (lo + hi) * f32(0.5), (hi - lo) * f32(0.5)
    k = n // 4
    box = mid + (rng.random((k, 3), dtype=f32) * 2 - 1) * half * f32(1.5)

    def on_surface(count):
        pick = rng.integers(0, len(T), count)
        b = rng.random((count, 2), dtype=f32); b = np.where(b.sum(1, keepdims=True) > 1, 1 - b, b)
        return T[pick, 0] + b[:, :1] * (T[pick, 1] - T[pick, 0]) + b[:, 1:] * (T[pick, 2] - T[pick, 0])
    surface = on_surface(k)
    d = rng.normal(size=(k, 3)).astype(f32)
    near = on_surface(k) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 1e-3, (k, 1)).astype(f32)
    far = rng.uniform(-8, 8, (n - 3 * k, 3)).astype(f32)
    return np.ascontiguousarray(np.concatenate([box, surface, near, far]), f32)


def reachable_triangles(bvh4, num_tris):
    """bool per triangle: a leaf of it is reached by the walk of build_wide_bvh (children that are out of range or whose box is degenerate,
    and everything below them, are not).  This restates the skip rules of csrc/pt_host.cpp::build_wide_bvh (empty slot: child == INVALID or
    >= numNodes; kDegenerate slot: any(mn > mx), false with a NaN) and the degenerate-root rule; if those change, this must follow."""
    b = np.asarray(bvh4, np.uint32)
    m = int(b[0])
    out = np.zeros(num_tris, bool)
    if m == 0:
        return out
    rec = b[1:1 + 8 * m].reshape(m, 8)
    w = rec[:, :3].astype(np.int64)
    h = np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF, w[:, 1] >> 16, w[:, 2] & 0xFFFF, w[:, 2] >> 16], -1)
    h = h.astype(np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        degenerate = np.any(h[:, :3] > h[:, 3:], -1)
    if degenerate[0]:
        return out
    stack = [0]
    while stack:
        i = stack.pop()
        if rec[i, 7] & LEAF:
            t = int(rec[i, 7] & 0x7FFFFFFF)
            if t < num_tris:
                out[t] = True
            continue
        for c in rec[i, 3:7]:
            if c != INVALID and c < m and not degenerate[c]:
                stack.append(int(c))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def closest_point_of(tris, prim, u, v):
    """v0 + u*e1 + v*e2 in f64 from the f32 edges the triangle record stores."""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(prim, np.int64)]
    e1 = (T[:, 1] - T[:, 0]).astype(np.float64); e2 = (T[:, 2] - T[:, 0]).astype(np.float64)
    return T[:, 0].astype(np.float64) + e1 * np.asarray(u, np.float64)[:, None] + e2 * np.asarray(v, np.float64)[:, None]


def deviations(points, tris, res, ref_dist):
    """The three deviations from the float64 minimum, in the same units: of dist, of the float64 distance of prim, of the (u, v) point."""
    dist, prim, u, v = res
    p = points[:, :3].astype(np.float64)
    d_prim = closestref.distance_to(p, tris, prim)
    d_point = np.linalg.norm(p - closest_point_of(tris, prim, u, v), axis=1)
    return np.abs(dist.astype(np.float64) - ref_dist), d_prim - ref_dist, np.abs(d_point - ref_dist)


def check_against_float64(points, tris, res, ref_dist, report=None):
    """The issue's check, no point excluded: everything is found (r_max = +inf, a non-empty reference), prim's float64 distance <= min + tol,
    |dist - min| <= tol, the (u, v) point lies within tol of the minimum, u, v >= 0 and u + v <= 1 + 2^-22."""
    dist, prim, u, v = res
    assert np.all(prim != MISS) and np.all(np.isfinite(ref_dist))
    tol = tolerance(points, tris)
    dev = deviations(points, tris, res, ref_dist)
    unit = tol / TOL_K
    worst = max(float(np.max(d)) for d in dev) / unit
    if report is not None:
        report.append(worst)
    print("closest points: largest deviation %.3f units of 2^-24 (max|p| + max|v|), tolerance %g units" % (worst, TOL_K))
    assert float(dev[1].max()) <= tol and float(dev[0].max()) <= tol and float(dev[2].max()) <= tol, worst
    assert np.all(u >= 0) and np.all(v >= 0) and np.all(u.astype(np.float64) + v.astype(np.float64) <= 1 + 2.0 ** -22)


def check_same_minimum(points, tris, a, b, d2_of):
    """dist bits equal on every point; prim equal, or the two prims have the same d2 bits (d2_of(points, prim) evaluates the product's d2)."""
    assert same_bits(a[0], b[0]), np.flatnonzero(bits(a[0]) != bits(b[0]))[:10]
    diff = np.flatnonzero(a[1] != b[1])
    if len(diff):
        assert np.all(a[1][diff] != MISS) and np.all(b[1][diff] != MISS)
        assert same_bits(d2_of(points[diff], a[1][diff]), d2_of(points[diff], b[1][diff])), diff[:10]


def product_uv_d2(points, tris, prim):
    """The product's f32 arithmetic (csrc/pt_closest.h) restated in numpy float32, operation by operation:
    returns (u, v, d2) of points[i] against triangle prim[i]."""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(prim, np.int64)]
    v0 = T[:, 0]; e1 = T[:, 1] - T[:, 0]; e2 = T[:, 2] - T[:, 0]
    ap = np.asarray(points, f32)[:, :3] - v0

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    with np.errstate(all="ignore"):
        a, b, c, d1, d2 = dot(e1, e1), dot(e1, e2), dot(e2, e2), dot(e1, ap), dot(e2, ap)
        ra = f32(1.0) / a; k = b * ra
        f = e2 - e1 * k[:, None]
        rf = f32(1.0) / dot(f, f)
        vq = dot(f, ap) * rf; uq = (d1 - vq * b) * ra
        cd, bd, ad, be = c - d2, b - d1, a - d1, b - d2
        inner = np.where(uq < 0, np.where(vq < 0, np.where(d1 > 0, 0, 1), 1), np.where(vq < 0, 0, 3))
        outer = np.where(uq < 0, np.where(cd > bd, 2, 1), np.where(vq < 0, np.where(ad > be, 2, 0), 2))
        where = np.where(uq + vq <= 1, inner, outer)
        num = np.choose(where, [d1, d2, cd - bd, cd - bd])
        den = np.choose(where, [a, c, (a - (b + b)) + c, (a - (b + b)) + c])
        r = f32(1.0) / den
        x = np.where(where == 0, d1 * ra, num * r)
        x = np.where(num <= 0, f32(0), np.where(num >= den, f32(1), x))
        zero = np.zeros_like(a)
        u = np.choose(where, [x, zero, x, uq])
        v = np.choose(where, [zero, x, f32(1.0) - x, vq])
        diff = ap - (e1 * u[:, None] + e2 * v[:, None])
        out = dot(diff, diff)
    assert out.dtype == f32
    return u, v, out


def product_d2(points, tris, prim):
    return product_uv_d2(points, tris, prim)[2]
