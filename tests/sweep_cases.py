"""Shared by the sphere-cast tests (tests/test_sweep_host.py, tests/test_gpu_sweep.py, tests/test_js_sweep.py): the input recipe, the
numpy-float32 restatement of csrc/pt_sweep.h operation for operation, the tolerance against the float64 reference (tests/sweepref.py) and
the checks."""
import numpy as np

import sweepref
from closest_cases import MISS, bits, product_uv_d2, same_bits

f32 = np.float32
INF = f32(np.inf)

# The tolerance unit is 2^-24 * (max|o| + max|vertex| + r) per item, tol = TOL_K units.  MEASURED_K is the smallest K at which the twin
# passes both checks that use tol in test_sweep_host.py, on every scene and tree: the sandwich against float64 passes from K = 1.0 on
# (tried in steps of 1/8: tetra fails at 0.875, every other scene passes at 0.5 or 1.0), the clearance at the reported time deviates by
# at most 2.67 units (soup1k after the refit; every other scene between 0.74 and 2.65).  TOL_K is four times the larger, rounded up to a
# power of two, as closest_cases.py does.  DESIGN.md section 22 repeats both.
MEASURED_K = 2.67
TOL_K = 16.0
WIDE_REL = 1e-4            # a sandwich is wide where t_ref(r - tol) - t_ref(r + tol) > WIDE_REL * extent / |d|, or exactly one side misses
WIDE_SHARE = 0.01          # at most this share of a scene's items may be wide


def extent_of(tris):
    v = np.asarray(tris, f32).reshape(-1, 3)
    return float((v.max(0) - v.min(0)).max())


def sweep_set(rt, tris, n, seed):
    """n PtSweep records by the recipe of DESIGN.md section 22: origins uniform in 1.5x the scene box; half the directions aimed at a
    triangle centroid, half at a uniform point of the box; radii drawn from {0, 0.2 %, 1 %, 5 %} of the extent; a quarter with a finite
    t_max (1: the sweep ends at its target; the directions are target - origin, so most are not unit length); another quarter with the
    direction scaled by a power of two in [1/4, 4]."""
    rng = np.random.default_rng(seed)
    T = np.asarray(tris, f32).reshape(-1, 3, 3)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    ext = extent_of(tris)
    org = (c + (rng.random((n, 3)) * 2 - 1) * 1.5 * h).astype(f32)
    cent = T[rng.integers(0, len(T), n)].mean(axis=1)
    unif = c + (rng.random((n, 3)) * 2 - 1) * h
    tgt = np.where((np.arange(n) % 2 == 0)[:, None], cent, unif).astype(f32)
    d = (tgt - org).astype(f32)
    scale = np.where(np.arange(n) % 4 == 1, 2.0 ** rng.integers(-2, 3, n), 1.0).astype(f32)
    d = (d * scale[:, None]).astype(f32)
    t_max = np.where(np.arange(n) % 4 == 3, f32(1.0), INF)
    radius = (np.array([0.0, 0.002, 0.01, 0.05])[rng.integers(0, 4, n)] * ext).astype(f32)
    return rt.pack_sweeps(org, d, radius, t_max)


def units(sweeps, tris):
    """the tolerance unit of every item: 2^-24 * (max|o| + max|vertex| + r)"""
    S = np.asarray(sweeps, np.float64).reshape(-1, 8)
    return 2.0 ** -24 * (np.abs(S[:, 0:3]).max(axis=1) + float(np.abs(np.asarray(tris, f32)).max()) + S[:, 7])


# ---- csrc/pt_sweep.h in numpy float32, operation for operation --------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _sel_min(a, b):
    return np.where(b < a, b, a)


def _sel_max(a, b):
    return np.where(b > a, b, a)


def safe_inv(d):
    with np.errstate(all="ignore"):
        return np.where(np.abs(d) > f32(1e-8), f32(1.0) / d, f32(1e30)).astype(f32)


def product_tT(o, d, r, tri):
    """Pairwise: o, d (k, 3), r (k,), tri (k, 3, 3) float32 -> t_T (k,) float32, +inf where the triangle is rejected (`best` = +inf: the
    comparison tmin < best only ever rejects a triangle whose t_T >= best)."""
    o = np.asarray(o, f32); d = np.asarray(d, f32); r = np.asarray(r, f32)
    v0 = tri[:, 0]; e1 = tri[:, 1] - tri[:, 0]; e2 = tri[:, 2] - tri[:, 0]
    with np.errstate(all="ignore"):
        inv = safe_inv(d)
        v1 = v0 + e1; v2 = v0 + e2
        mn = _sel_min(_sel_min(v0, v1), v2); mx = _sel_max(_sel_max(v0, v1), v2)
        a = (mn - (o + r[:, None])) * inv; b = (mx - (o - r[:, None])) * inv
        neg = inv < 0
        near = np.where(neg, b, a); far = np.where(neg, a, b)
        tmin = _sel_max(_sel_max(near[:, 0], near[:, 1]), near[:, 2]); tmax = _sel_min(_sel_min(far[:, 0], far[:, 1]), far[:, 2])
        t_in = np.where(tmin > 0, tmin, f32(0))
        box_ok = (tmax >= t_in) & (tmin < INF)
        s = o - v0
        _, _, d2 = _uv_d2(s, e1, e2)
        rr = r * r
        # face
        n = _cross(e1, e2)
        nn, h, nd = _dot(n, n), _dot(n, s), _dot(n, d)
        rn = r * np.sqrt(nn)
        tf = (np.where(h >= 0, rn, -rn) - h) / nd
        w = s + d * tf[:, None]
        ga, gb = _dot(e1, e1), _dot(e1, e2)
        ra = f32(1.0) / ga; k = gb * ra
        g = e2 - e1 * k[:, None]
        rf = f32(1.0) / _dot(g, g)
        vq = _dot(g, w) * rf; uq = (_dot(e1, w) - vq * gb) * ra
        tc = np.where((tf >= 0) & (uq >= 0) & (vq >= 0) & (uq + vq <= 1), tf, INF)
        m1 = o - v1; m2 = o - v2

        def edge(tc, m, e):
            p = _cross(m, e); q = _cross(d, e)
            ee = _dot(e, e)
            rA = f32(1.0) / _dot(q, q)
            t0 = -(_dot(p, q) * rA)
            ww = p + q * t0[:, None]
            t = t0 - np.sqrt((rr * ee - _dot(ww, ww)) * rA)
            gg = _dot(m, e) + t * _dot(d, e)
            return np.where((t >= 0) & (gg >= 0) & (gg <= ee) & (t < tc), t, tc)

        def vertex(tc, m):
            t0 = -(_dot(m, d) * rdd)
            ww = m + d * t0[:, None]
            t = t0 - np.sqrt((rr - _dot(ww, ww)) * rdd)
            return np.where((t >= 0) & (t < tc), t, tc)
        tc = edge(tc, s, e1); tc = edge(tc, s, e2); tc = edge(tc, m1, e2 - e1)
        rdd = f32(1.0) / _dot(d, d)
        tc = vertex(tc, s); tc = vertex(tc, m1); tc = vertex(tc, m2)
        tc = np.where(d2 <= rr, f32(0), tc)
        tT = np.where(tc > t_in, tc, t_in)
    out = np.where(box_ok, tT, INF)
    assert out.dtype == f32
    return out


def _uv_d2(ap, e1, e2):
    """closest_cases.product_uv_d2 on ap = p - v0 directly (a triangle at the origin: v0 = 0 leaves ap's bits alone)"""
    k = len(ap)
    tri = np.stack([np.zeros((k, 3), f32), e1, e2], 1)
    return product_uv_d2(ap, tri.reshape(-1), np.arange(k))


def product_sweep(sweeps, tris, budget=1 << 18):
    """The brute-force product in numpy float32: (t, prim, u, v) of every sweep over every triangle in index order."""
    S = np.asarray(sweeps, f32).reshape(-1, 8)
    T = np.asarray(tris, f32).reshape(-1, 3, 3)
    n, m = len(S), len(T)
    t = np.full(n, INF, f32); prim = np.full(n, MISS, np.uint32)
    step = max(1, budget // max(m, 1))
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step); k = i1 - i0
        tt = product_tT(np.repeat(S[i0:i1, 0:3], m, axis=0), np.repeat(S[i0:i1, 4:7], m, axis=0), np.repeat(S[i0:i1, 7], m),
                        np.tile(T, (k, 1, 1))).reshape(k, m)
        with np.errstate(invalid="ignore"):
            tt = np.where(tt == tt, tt, INF)                                      # a NaN is never accepted
        j = tt.argmin(axis=1); best = tt[np.arange(k), j]
        hit = best < S[i0:i1, 3]
        t[i0:i1] = np.where(hit, best, INF); prim[i0:i1] = np.where(hit, j, MISS)
    walked = sweeps_walked(S)
    t[~walked] = INF; prim[~walked] = MISS
    u, v = contact_uv(S, T, t, prim)
    return t, prim, u, v


def sweeps_walked(S):
    S = np.asarray(S, f32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(S).any(axis=1) & (S[:, 3] > 0) & (S[:, 7] >= 0) & (S[:, 4:7] != 0).any(axis=1)


def contact_point(S, t):
    """c = fl(o + fl(t * d)) per component, float32"""
    S = np.asarray(S, f32).reshape(-1, 8)
    with np.errstate(all="ignore"):
        return (S[:, 0:3] + np.asarray(t, f32)[:, None] * S[:, 4:7]).astype(f32)


def contact_uv(S, tris, t, prim):
    """u, v of closest_cases.product_uv_d2 for c against the winning record; 0, 0 on a miss"""
    hit = prim != MISS
    u = np.zeros(len(prim), f32); v = np.zeros(len(prim), f32)
    if hit.any():
        c = contact_point(np.asarray(S, f32).reshape(-1, 8)[hit], np.asarray(t, f32)[hit])
        u[hit], v[hit], _ = product_uv_d2(c, np.asarray(tris, f32).reshape(-1), prim[hit])
    return u, v


def check_same_minimum(sweeps, tris, a, b):
    """t, u, v bits equal on every item -- unless prim differs, which is allowed only between triangles with equal t_T bits (then u, v are
    each checked against their own prim by check_uv)."""
    assert same_bits(a[0], b[0]), np.flatnonzero(bits(a[0]) != bits(b[0]))[:10]
    diff = np.flatnonzero(a[1] != b[1])
    same = a[1] == b[1]
    assert same_bits(a[2][same], b[2][same]) and same_bits(a[3][same], b[3][same])
    if len(diff):
        assert np.all(a[1][diff] != MISS) and np.all(b[1][diff] != MISS)
        S = np.asarray(sweeps, f32).reshape(-1, 8)[diff]
        T = np.asarray(tris, f32).reshape(-1, 3, 3)
        ta = product_tT(S[:, 0:3], S[:, 4:7], S[:, 7], T[a[1][diff].astype(np.int64)])
        tb = product_tT(S[:, 0:3], S[:, 4:7], S[:, 7], T[b[1][diff].astype(np.int64)])
        assert same_bits(ta, tb), diff[:10]


def check_uv(sweeps, tris, res):
    u, v = contact_uv(sweeps, tris, res[0], res[1])
    assert same_bits(u, res[2]) and same_bits(v, res[3])


def reference_band(sweeps, tris, k=TOL_K):
    """(t_lo, t_hi, tau_of, wide): t_ref(r + tol), t_ref(max(r - tol, 0)) and the wide flags, from the float64 reference alone."""
    S = np.asarray(sweeps, np.float64).reshape(-1, 8)
    tol = k * units(sweeps, tris)
    t_lo, _ = sweepref.t_ref(sweeps, tris, S[:, 7] + tol)
    t_hi, _ = sweepref.t_ref(sweeps, tris, np.maximum(S[:, 7] - tol, 0.0))
    dn = np.linalg.norm(S[:, 4:7], axis=1)
    with np.errstate(invalid="ignore"):
        wide = (np.isfinite(t_lo) != np.isfinite(t_hi)) | (np.nan_to_num(t_hi - t_lo, nan=0.0, posinf=0.0) > WIDE_REL * extent_of(tris) / dn)
    return t_lo, t_hi, tol, wide


def sandwich_violation(sweeps, tris, t, band):
    """The largest violation of t_ref(r + tol) - tau <= t <= t_ref(max(r - tol, 0)) + tau over the items (<= 0: none), with
    tau = tol / |d| + 4 * 2^-24 * t; a hit only where t_ref(r + tol) hits, a miss only where t_ref(max(r - tol, 0)) misses; the upper side
    is not checked for items with r <= tol."""
    S = np.asarray(sweeps, np.float64).reshape(-1, 8)
    t_lo, t_hi, tol, _ = band
    t = np.asarray(t, np.float64)
    hit = np.isfinite(t)
    dn = np.linalg.norm(S[:, 4:7], axis=1)
    tau = tol / dn + 4 * 2.0 ** -24 * np.where(hit, t, 0.0)
    upper = S[:, 7] > tol
    bad_hit = hit & ~np.isfinite(t_lo)
    bad_miss = ~hit & np.isfinite(t_hi) & upper
    worst = -np.inf
    if bad_hit.any() or bad_miss.any():
        return np.inf
    with np.errstate(invalid="ignore"):
        low = np.where(hit, (t_lo - tau) - t, -np.inf)
        high = np.where(hit & upper & np.isfinite(t_hi), t - (t_hi + tau), -np.inf)
    worst = max(worst, float(low.max(initial=-np.inf)), float(high.max(initial=-np.inf)))
    return worst
