"""Shared by the box-overlap tests (tests/test_box_host.py, tests/test_gpu_box.py, tests/box_torch_cases.py, the audits): the box sets, the
numpy float32 restatement of csrc/pt_overlap.h, the float64 separating-axis reference with its margin, and the comparisons of lists
(include/mi355pt.h pt_box_search)."""
import ctypes as C

import numpy as np

import closest_cases as clc
import radius_cases as rc
import crossing_cases as cc
from radius_cases import GUARD, assert_truncation, extent, owner      # noqa: F401  (re-exported: the list queries share them)
from scenes import comb_bvh4

f32 = np.float32
N_BOXES = 500
BOX_SEED = 7
H_LO, H_HI = 0.01, 0.1          # half-extents are drawn per axis from [H_LO, H_HI] x the scene extent
BAND_CAP = 0.005                # the tolerance band may hold at most 0.5 % of the listed pairs


# crossing_cases.comb_tree() has 30 levels with the chain child in a random slot.  A box query walks passing children depth first in slot
# order, so only the leaves BEHIND the chain child's slot wait on the stack while the chain is walked: 1.5 per level on average, 50 entries
# for a box that holds the whole comb (measured; no smaller box stacks more) -- below the cap of 64.  The same comb with 64 levels overruns it.
DEEP_COMB_LEVELS = 64


def deep_comb():
    """(triangles, bvh4) of the comb with DEEP_COMB_LEVELS levels"""
    return comb_bvh4(DEEP_COMB_LEVELS, cc.COMB_SEED)


def install(rt, orc, ctx, name):
    """radius_cases.install, and "deepcomb"; returns (triangles, the BVH4 the context holds: what the host twin walks)."""
    if name != "deepcomb":
        return rc.install(rt, orc, ctx, name)
    tris, b4 = deep_comb()
    ctx.set_triangles(tris); ctx.set_bvh4(b4)
    return tris, ctx.read_bvh4()


def box_records(rt, tris, n=N_BOXES, seed=BOX_SEED):
    """(n, 8) PtBox records: half with centres uniform in 1.5 x the scene box, half at triangle centroids; half-extents per axis uniform in
    [H_LO, H_HI] x the scene extent; computed in float64, the corners rounded to f32."""
    rng = np.random.default_rng(seed)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)
    lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
    mid, half = (lo + hi) * 0.5, (hi - lo) * 0.5
    k = n // 2
    uniform = mid + (rng.random((k, 3)) * 2 - 1) * half * 1.5
    centroid = T[rng.integers(0, len(T), n - k)].mean(1)
    c = np.concatenate([uniform, centroid])
    h = rng.uniform(H_LO, H_HI, (n, 3)) * extent(tris)
    return rt.pack_boxes((c - h).astype(f32), (c + h).astype(f32))


def whole_scene_box(rt, tris, n=1):
    """n copies of one box that holds the whole scene with room to spare"""
    v = np.asarray(tris, f32).reshape(-1, 3)
    lo, hi = v.min(0) - f32(0.5), v.max(0) + f32(0.5)
    return rt.pack_boxes(np.tile(lo, (n, 1)), np.tile(hi, (n, 1)))


def walked(boxes):
    b = np.asarray(boxes, f32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b[:, [0, 1, 2, 4, 5, 6]]).all(1) & (b[:, 0:3] <= b[:, 4:7]).all(1)


def words(res):
    """(offsets, prim, verts_inside) -> (offsets as int64, (m, 2) uint32 entry words)"""
    offsets, prim, inside = res[:3]
    return np.asarray(offsets).astype(np.int64), np.stack([np.asarray(prim, np.uint32), np.asarray(inside, np.uint32)], axis=1)


def keys(res):
    """(box << 32 | prim) of every entry"""
    off, ent = words(res)
    return (owner(off).astype(np.int64) << 32) | ent[:, 0]


def assert_same_lists(a, b, ordered):
    """Two results hold the same lists, entries word for word: in the same order, or as sets (each list sorted by prim)."""
    (oa, ea), (ob, eb) = words(a), words(b)
    assert np.array_equal(oa, ob), np.flatnonzero(oa != ob)[:10]
    if not ordered:
        ea, eb = ea[np.lexsort((ea[:, 0], owner(oa)))], eb[np.lexsort((eb[:, 0], owner(ob)))]
    assert np.array_equal(ea, eb), np.flatnonzero((ea != eb).any(1))[:10]


def assert_subset(walk, brute):
    """Every entry of `walk` is in `brute`'s list of the same box, word for word; returns how many of brute's entries are missing."""
    (ow, ew), (ob, eb) = words(walk), words(brute)
    kw, kb = keys(walk), keys(brute)
    assert len(np.unique(kw)) == len(kw)                                   # no triangle twice in a list
    order = np.argsort(kb)
    pos = np.searchsorted(kb[order], kw)
    assert np.all(pos < max(len(kb), 1)) and np.array_equal(kb[order][np.minimum(pos, len(kb) - 1)], kw)
    assert np.array_equal(eb[order][pos], ew)
    return len(kb) - len(kw)


# ---- csrc/pt_overlap.h restated in numpy float32, operation for operation ---------------------------------------------------------------
def _records(tris, ti):
    """v0, e1, e2 of the triangle records (csrc/pt_host.cpp::build_tri_records): the edges are f32 differences of the vertices"""
    T = np.asarray(tris, f32).reshape(-1, 3, 3)[np.asarray(ti, np.int64)]
    return T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]


def product_axes(boxes, tris, bi, ti):
    """(a) of the triangle test for the pairs (bi[j], ti[j]): -> (passes, verts_inside, (v0, v1, v2, e1, e2))"""
    b = np.asarray(boxes, f32)
    lo, hi = b[bi, 0:3], b[bi, 4:7]
    v0, e1, e2 = _records(tris, ti)
    with np.errstate(all="ignore"):
        v1, v2 = v0 + e1, v0 + e2
        le = [v <= hi for v in (v0, v1, v2)]
        ge = [v >= lo for v in (v0, v1, v2)]
    a = ((le[0] | le[1] | le[2]) & (ge[0] | ge[1] | ge[2]) & (le[0] | ge[0]) & (le[1] | ge[1]) & (le[2] | ge[2])).all(1)
    inside = [(l & g).all(1) for l, g in zip(le, ge)]
    vin = inside[0].astype(np.uint32) | (inside[1].astype(np.uint32) << 1) | (inside[2].astype(np.uint32) << 2)
    return a, vin, (v0, v1, v2, e1, e2)


def product_overlap(boxes, tris, bi, ti):
    """The whole triangle test for the pairs (bi[j], ti[j]): -> (accepted, verts_inside)"""
    b = np.asarray(boxes, f32)
    lo, hi = b[bi, 0:3], b[bi, 4:7]
    a, vin, (v0, v1, v2, e1, e2) = product_axes(boxes, tris, bi, ti)
    half = f32(0.5)
    with np.errstate(all="ignore"):
        c, h = (lo + hi) * half, (hi - lo) * half
        a0, a1, a2 = v0 - c, v1 - c, v2 - c
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        d = (nx * a0[:, 0] + ny * a0[:, 1]) + nz * a0[:, 2]
        r = (np.abs(nx) * h[:, 0] + np.abs(ny) * h[:, 1]) + np.abs(nz) * h[:, 2]
        plane = np.abs(d) <= r

        def axis(p0, p1, p2, rr):
            m = -rr
            return ((p0 <= rr) | (p1 <= rr) | (p2 <= rr)) & ((p0 >= m) | (p1 >= m) | (p2 >= m))
        edges = np.ones(len(bi), bool)
        for f in (e1, e2 - e1, e2):
            g = np.abs(f)
            X, Y, Z = 0, 1, 2
            edges &= axis(*[q[:, Z] * f[:, Y] - q[:, Y] * f[:, Z] for q in (a0, a1, a2)], h[:, Y] * g[:, Z] + h[:, Z] * g[:, Y])
            edges &= axis(*[q[:, X] * f[:, Z] - q[:, Z] * f[:, X] for q in (a0, a1, a2)], h[:, X] * g[:, Z] + h[:, Z] * g[:, X])
            edges &= axis(*[q[:, Y] * f[:, X] - q[:, X] * f[:, Y] for q in (a0, a1, a2)], h[:, X] * g[:, Y] + h[:, Y] * g[:, X])
    assert d.dtype == f32 and r.dtype == f32
    return a & ((vin != 0) | (plane & edges)), vin


def numpy_brute(boxes, tris, chunk_pairs=1 << 21):
    """The brute-force list restated in numpy float32: every triangle in index order through product_overlap.  (a) runs on every pair; (b)
    and (c) on the pairs that pass it, which is every pair that can be accepted.  Returns (offsets, prim, verts_inside)."""
    b = np.asarray(boxes, f32)
    n, m = len(b), np.asarray(tris).size // 9
    ok = walked(b)
    counts = np.zeros(n, np.int64)
    prims, vins = [], []
    step = max(1, chunk_pairs // max(m, 1))
    for s in range(0, n, step):
        sel = np.arange(s, min(s + step, n))
        sel = sel[ok[sel]]
        if not len(sel) or not m:
            continue
        bi = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        a, _, _ = product_axes(b, tris, bi, ti)
        bi, ti = bi[a], ti[a]
        acc, vin = product_overlap(b, tris, bi, ti)
        counts += np.bincount(bi[acc], minlength=n)
        prims.append(ti[acc].astype(np.uint32)); vins.append(vin[acc])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return offsets, cat(prims), cat(vins)


# ---- the float64 reference: separating axes, normalised --------------------------------------------------------------------------------
def tolerance(boxes, tris):
    b = np.asarray(boxes, f32)[:, [0, 1, 2, 4, 5, 6]]
    return clc.TOL_K * 2.0 ** -24 * (float(np.abs(b[np.isfinite(b).all(1)]).max()) + float(np.abs(tris).max()))


def margin64(boxes, tris, bi, ti):
    """g of the pairs (bi[j], ti[j]) in float64 from the vertices and corners themselves: the maximum over the 13 axes (three box axes, the
    triangle's normal, nine edge x box-axis products) of the gap between the two projections divided by the axis' length, axes of length
    zero skipped.  g > 0: separated by g; g < 0: the projections overlap by at least -g on every axis."""
    b = np.asarray(boxes, f32).astype(np.float64)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)[np.asarray(ti, np.int64)]
    c, h = (b[bi, 0:3] + b[bi, 4:7]) * 0.5, (b[bi, 4:7] - b[bi, 0:3]) * 0.5
    V = T - c[:, None, :]
    E = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
    eye = np.eye(3)
    axes = [np.broadcast_to(eye[k], (len(bi), 3)) for k in range(3)] + [np.cross(E[:, 0], E[:, 1])]
    axes += [np.cross(np.broadcast_to(eye[k], (len(bi), 3)), E[:, j]) for j in range(3) for k in range(3)]
    g = np.full(len(bi), -np.inf)
    for L in axes:
        ln = np.linalg.norm(L, axis=1)
        p = np.einsum("nic,nc->ni", V, L)
        r = (np.abs(L) * h).sum(1)
        gap = np.maximum(p.min(1) - r, -r - p.max(1))
        with np.errstate(all="ignore"):
            g = np.where(ln > 0, np.maximum(g, gap / ln), g)
    return g


def check_against_float64(boxes, tris, res):
    """The issue's check: every pair with g < -tol is listed, no pair with g > tol is listed; returns (pairs inside the band, listed)."""
    b = np.asarray(boxes, f32)
    m = np.asarray(tris).size // 9
    tol = tolerance(b, tris)
    have = keys(res)
    band = 0
    sel_all = np.flatnonzero(walked(b))
    step = max(1, (1 << 20) // max(m, 1))
    for s in range(0, len(sel_all), step):
        sel = sel_all[s:s + step]
        bi = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        g = margin64(b, tris, bi, ti)
        k = (bi.astype(np.int64) << 32) | ti
        listed = np.isin(k, have)
        assert np.all(listed[g < -tol]), ("missing", bi[(g < -tol) & ~listed][:5], ti[(g < -tol) & ~listed][:5])
        assert not np.any(listed[g > tol]), ("phantom", bi[(g > tol) & listed][:5], ti[(g > tol) & listed][:5])
        band += int((np.abs(g) <= tol).sum())
    return band, len(have)


# ---- raw calls with a guard behind the entries ------------------------------------------------------------------------------------------
def raw_search(rt, fn, head, boxes, flags, capacity, null_entries=False, tail=()):
    """One call of a pt_box_search* entry point with a guard pattern in every entry: `fn(*head, boxes, n, flags, offsets, entries, capacity,
    *tail)`.  The entry buffer holds capacity + 8 records.  Returns (status, offsets, (capacity + 8, 4) uint32 records)."""
    n = len(boxes)
    offsets = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    entries = rt._aligned_zeros((capacity + 8, 4), np.uint32)
    entries[...] = GUARD
    st = fn(*head, boxes.ctypes.data_as(C.POINTER(rt.PtBox)), C.c_uint64(n), C.c_uint32(flags), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            None if null_entries else entries.ctypes.data_as(C.POINTER(rt.PtOverlap)), C.c_uint64(capacity), *tail)
    return st, offsets, entries


def records_of(res):
    """(offsets, prim, verts_inside) -> the (m, 4) uint32 PtOverlap records, reserved words 0"""
    _, ent = words(res)
    return np.concatenate([ent, np.zeros_like(ent)], axis=1)


# ---- the exact cases of the issue, on the triangle (0,0,0), (1,0,0), (0,1,0) ------------------------------------------------------------
EXACT_TRI = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], f32)
_E = 2.0 ** -20
EXACT = [   # (lo, hi, listed, verts_inside)
    ([1, 0, -1], [2, 1, 1], True, 2),                                   # holds vertex 1 alone
    ([0.5, 0.5, -1], [2, 2, 1], True, 0),                               # touches the hypotenuse
    ([0.5 + _E, 0.5 + _E, -1], [2, 2, 1], False, 0),                    # 2^-20 off it
    ([-1, -1, 0], [2, 2, 0], True, 7),                                  # a rectangle in the triangle's plane
    ([0.5, 0.5, 0], [2, 2, 0], True, 0),                                # the same, touching the hypotenuse
    ([-1, -1, _E], [2, 2, 1], False, 0),                                # 2^-20 above the plane
    ([0.25, 0.25, 0], [0.25, 0.25, 0], True, 0),                        # a point box on the face
    ([-1, -1, -1], [2, 2, 2], True, 7),                                 # holds all three vertices
]


def exact_boxes(rt):
    return rt.pack_boxes([e[0] for e in EXACT], [e[1] for e in EXACT])


def assert_exact(res):
    off, ent = words(res)
    assert np.diff(off).tolist() == [int(e[2]) for e in EXACT], np.diff(off)
    assert ent[:, 0].tolist() == [0] * len(ent) and ent[:, 1].tolist() == [e[3] for e in EXACT if e[2]], ent


# ---- the audit: a box around every aimed position of every triangle ----------------------------------------------------------------------
AUDIT_EPS = 2.0                 # half-extent of an audit box, in tolerances


def aimed_boxes(rt, tris):
    """-> ((4 n, 8) PtBox records, the triangle each is aimed at): p +- eps around the four aimed positions of every triangle
    (treeaudit.aimed_rays: the centroid and three points near the corners, float64 points of the triangle itself).  eps is AUDIT_EPS
    tolerances of the float64 check -- 32 units of 2^-24 (max|box| + max|vertex|), a few ulps of a coordinate at the scene's scale: the
    box reaches 2 tol across the triangle's plane and past every edge axis, so by that check's own rule (g < -tol) the pair must be listed."""
    import treeaudit as ta
    rays = ta.aimed_rays(tris)
    eps = AUDIT_EPS * clc.TOL_K * 2.0 ** -24 * (float(np.abs(rays.P).max()) + float(np.abs(tris).max()))
    return rt.pack_boxes((rays.P - eps).astype(f32), (rays.P + eps).astype(f32)), rays.tri


def assert_audited(res, tri, name):
    """every box lists the triangle it is aimed at, with no exception"""
    have = keys(res)
    want = (np.arange(len(tri), dtype=np.int64) << 32) | np.asarray(tri, np.int64)
    lost = ~np.isin(want, have)
    assert not lost.any(), "%s: %d of %d aimed boxes do not list their triangle, first triangles %s" % (name, int(lost.sum()), len(tri), np.asarray(tri)[lost][:10])
