"""Shared by the k-nearest tests (tests/test_knn_host.py, tests/test_gpu_knn.py, tests/knn_torch_cases.py): the point sets, the numpy
restatement of the brute-force rows, the list rule in python, a float64 statement of the k smallest distances, and the comparisons of rows
(include/mi355pt.h pt_nearest_k)."""
import numpy as np

import closest_cases as clc
import closestref
import radius_cases as rc
from scenes import TETRA

f32 = np.float32
N_POINTS = 500
POINT_SEED = 17
KS = (1, 2, 5, 16, 64)
K_MAX = 64
RADII = ("inf", "drawn")        # r_max = +inf, and one radius per point drawn from 1-10 % of the extent (radius_cases.point_records)
INF_BITS = 0x7F800000
PAD = np.array([INF_BITS, 0xFFFFFFFF, 0, 0], np.uint32)

DOUBLED_TETRA = np.concatenate([TETRA.reshape(-1), TETRA.reshape(-1)]).astype(f32)      # every triangle twice: exact ties


def point_records(rt, tris, radii, n=N_POINTS, seed=POINT_SEED):
    """(n, 4) PtPoint records of closest_cases.query_points: radii "inf" or "drawn"."""
    if radii == "inf":
        return rt.pack_points(clc.query_points(tris, n, seed), np.inf)
    return rc.point_records(rt, tris, n=n, seed=seed)


def words(res):
    """(dist, prim, u, v), each (n, k) -> (n, k, 4) uint32 records"""
    dist, prim, u, v = (np.asarray(a) for a in res[:4])
    return np.stack([clc.bits(dist.reshape(-1)).reshape(dist.shape), prim.astype(np.uint32), clc.bits(u.reshape(-1)).reshape(u.shape),
                     clc.bits(v.reshape(-1)).reshape(v.shape)], axis=2)


def listed(w):
    """(n, k) bool: the entries that are no padding; asserts that the padding is whole and sits behind the listed entries"""
    m = w[:, :, 1] != 0xFFFFFFFF
    assert np.all(w[~m] == PAD)
    assert np.all(m[:, :-1] >= m[:, 1:])
    return m


def assert_same_rows(a, b):
    wa, wb = words(a), words(b)
    assert wa.shape == wb.shape, (wa.shape, wb.shape)
    assert np.array_equal(wa, wb), np.flatnonzero((wa != wb).any(axis=(1, 2)))[:10]


def numpy_rows(points, tris, kmax=K_MAX, chunk_pairs=1 << 20):
    """The brute-force rows restated in numpy float32 (closest_cases.product_uv_d2 on every point-triangle pair): per point the kmax
    smallest d2 < r2 in ascending order, equal d2 in index order (a stable sort), dist = sqrt(d2), padded.  Returns (n, kmax, 4) uint32.
    The row for a smaller k is its first k entries: brute force meets the triangles in index order."""
    pts = np.asarray(points, f32)
    n, m = len(pts), np.asarray(tris).size // 9
    out = np.tile(PAD, (n, kmax, 1))
    walked = ~np.isnan(pts).any(1) & (pts[:, 3] > 0)
    with np.errstate(over="ignore"):
        r2 = pts[:, 3] * pts[:, 3]
    step = max(1, chunk_pairs // max(m, 1))
    for s in range(0, n, step):
        sel = np.arange(s, min(s + step, n))
        sel = sel[walked[sel]]
        if not len(sel) or not m:
            continue
        pi = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        u, v, d2 = clc.product_uv_d2(pts[pi], tris, ti)
        with np.errstate(invalid="ignore"):
            keep = d2 < r2[pi]
        key = np.where(keep, d2, f32(np.inf)).reshape(len(sel), m)
        order = np.argsort(key, axis=1, kind="stable")[:, :kmax]
        take = np.take_along_axis(keep.reshape(len(sel), m), order, axis=1)
        flat = (np.arange(len(sel))[:, None] * m + order)
        rec = np.stack([clc.bits(np.sqrt(d2[flat].astype(f32)).reshape(-1)).reshape(flat.shape), order.astype(np.uint32),
                        clc.bits(u[flat].reshape(-1)).reshape(flat.shape), clc.bits(v[flat].reshape(-1)).reshape(flat.shape)], axis=2)
        kk = rec.shape[1]
        out[sel, :kk] = np.where(take[:, :, None], rec, PAD)
    return out


def list_rule(sequence, k, r2=np.inf):
    """The list rule of the specification over a visit sequence [(d2 as float32, tag)]: accepted when d2 < worst2, inserted behind every
    pair with d2' <= d2, the pair behind the k-th falls off.  Returns the list."""
    lst = []
    for d2, tag in sequence:
        worst2 = r2 if len(lst) < k else lst[-1][0]
        if not d2 < worst2:
            continue
        j = len(lst)
        while j > 0 and lst[j - 1][0] > d2:
            j -= 1
        lst.insert(j, (d2, tag))
        del lst[k:]
    return lst


def radius_entries_by_prim(rt, tris, pts, chunk_entries=1 << 22):
    """Yields (first point, last point + 1, keys, entries) of radius_search_bvh4(brute_force=True) at the points' own r_max, a few points at
    a time so that a whole-scene radius does not list everything at once: keys = local point << 32 | prim, ascending."""
    m = np.asarray(tris).size // 9
    step = max(1, chunk_entries // max(m, 1))
    for s in range(0, len(pts), step):
        sub = np.ascontiguousarray(pts[s:s + step])
        off, ent = rc.words(rt.radius_search_bvh4(tris, None, sub, brute_force=True))
        keys = (rc.owner(off).astype(np.int64) << 32) | ent[:, 1]
        assert np.all(np.diff(keys) > 0)
        yield s, s + len(sub), keys, ent


def assert_entries_are_radius_entries(rt, tris, pts, rows):
    """Every listed (prim, dist, u, v) of every result in `rows` (a list of (n, k, 4) records) equals that prim's entry in
    radius_search_bvh4(brute_force=True) at the same r_max: it is a true record of a triangle with d2 < r2."""
    for lo, hi, keys, ent in radius_entries_by_prim(rt, tris, pts):
        for w in rows:
            sub = w[lo:hi]
            pi, j = np.nonzero(sub[:, :, 1] != 0xFFFFFFFF)
            rec = sub[pi, j]
            want = (pi.astype(np.int64) << 32) | rec[:, 1]
            pos = np.searchsorted(keys, want)
            assert np.all(pos < len(keys)) and np.array_equal(keys[np.minimum(pos, len(keys) - 1)], want)
            assert np.array_equal(ent[pos], rec)


def assert_distinct_prims(w):
    """the prims of a row are pairwise distinct (the padding aside)"""
    p = np.sort(np.where(w[:, :, 1] == 0xFFFFFFFF, np.arange(w.shape[1], dtype=np.int64)[None, :] + (1 << 40), w[:, :, 1].astype(np.int64)), axis=1)
    assert np.all(np.diff(p, axis=1) > 0)


def smallest_float64(points, tris, kmax=K_MAX, block=32):
    """Per point the kmax smallest float64 distances over ALL triangles, ascending, padded with +inf: (n, kmax).  A triangle lies inside
    the sphere around its centroid through its farthest vertex, so |p - c| - rad <= d <= |p - c| + rad: at least kmax triangles lie within
    the kmax-th smallest upper bound, and only triangles whose lower bound is within it are evaluated (closestref.closest_on_triangles)."""
    p = np.asarray(points, np.float64)[:, :3]
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    m = len(T)
    kk = min(kmax, m)
    cen = T.mean(1); rad = np.linalg.norm(T - cen[:, None, :], axis=2).max(1)
    out = np.full((len(p), kmax), np.inf)
    for s in range(0, len(p), block):
        q = p[s:s + block]
        ok = ~np.isnan(q).any(1)
        dc = np.linalg.norm(np.where(ok[:, None], q, 0.0)[:, None, :] - cen[None, :, :], axis=2)
        cutoff = np.partition(dc + rad[None, :], kk - 1, axis=1)[:, kk - 1]
        pi, ti = np.nonzero((dc - rad[None, :] <= cutoff[:, None]) & ok[:, None])
        d = closestref.closest_on_triangles(q[pi], T[ti])[0]
        order = np.lexsort((d, pi))
        pi, d = pi[order], d[order]
        start = np.searchsorted(pi, np.arange(len(q)))
        rank = np.arange(len(pi)) - start[pi]
        sel = rank < kk
        out[s + pi[sel], rank[sel]] = d[sel]
    return out


def comb_points(rt, n):
    """above the comb, r_max = +inf: the walk runs into the 64-entry cap (radius_cases / test_gpu_radius.points_for)"""
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.0, 2.0, n)], axis=1).astype(f32)
    return rt.pack_points(p, np.inf)


def guarded(rt, n, k, extra=8):
    """an aligned (n * k + extra, 4) uint32 buffer filled with radius_cases.GUARD"""
    buf = rt._aligned_zeros((n * k + extra, 4), np.uint32)
    buf[...] = rc.GUARD
    return buf


def assert_guard(buf, n, k):
    """every record before n * k was overwritten, the guard behind them is intact"""
    assert not np.any(np.all(buf[:n * k] == rc.GUARD, axis=1))
    assert np.all(buf[n * k:] == rc.GUARD)
