"""Shared by the triangle-overlap tests (tests/test_tri_host.py, tests/test_tri_pins.py, tests/test_gpu_tri.py, tests/tri_torchroute_cases.py):
the caller triangle sets, the float64 sandwich around triref's margin, the exact cases and the raw calls (include/mi355pt.h pt_tri_search,
DESIGN.md section 23).  The comparisons of lists are box_cases': an entry is two words there as well (prim, edges)."""
import ctypes as C

import numpy as np

import closest_cases as clc
import triref
from box_cases import BAND_CAP, assert_same_lists, assert_subset, install, keys, records_of, words      # noqa: F401  (re-exported)
from radius_cases import GUARD, assert_truncation, extent, owner                                          # noqa: F401

f32 = np.float32
N_TRIS = 500
TRI_SEED = 7
J_LO, J_HI = 0.01, 0.1          # the vertex jitter of a caller triangle is drawn from [J_LO, J_HI] x the scene extent
# The smallest K (in units of 2^-24 (max|caller coordinate| + max|vertex|)) from which the float64 sandwich holds on the host twin, over
# the 24 scene-tree pairs of test_tri_host.py: no listed pair has G < 0 and no unlisted pair G > 0 beyond it.  TOL_K = 16 is what is asserted.
MEASURED_K = 0.0


def caller_records(rt, tris, n=N_TRIS, seed=TRI_SEED, jitter=(J_LO, J_HI)):
    """(n, 12) PtTri records: each centred at the centroid of a random mesh triangle, its three vertices moved off the centre by up to
    s per axis, s per triangle uniform in `jitter` x the scene extent; computed in float64, rounded to f32."""
    rng = np.random.default_rng(seed)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)
    c = T[rng.integers(0, len(T), n)].mean(1)
    s = rng.uniform(jitter[0], jitter[1], n) * extent(tris)
    return rt.pack_tris((c[:, None, :] + (rng.random((n, 3, 3)) * 2 - 1) * s[:, None, None]).astype(f32))


def whole_scene_tri(rt, tris, n=1):
    """n copies of one caller triangle whose bounding box holds the whole scene, cutting through its middle"""
    v = np.asarray(tris, f32).reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64) - 0.5, v.max(0).astype(np.float64) + 0.5
    q = np.array([[lo[0], lo[1], lo[2]], [2 * hi[0] - lo[0], lo[1], hi[2]], [lo[0], 2 * hi[1] - lo[1], hi[2]]])
    return rt.pack_tris(np.tile(q, (n, 1, 1)).astype(f32))


def bounding_boxes(rt, rec):
    """the PtBox records of the caller triangles' exact bounding boxes"""
    Q = triref.callers(rec)
    return rt.pack_boxes(Q.min(1), Q.max(1))


# ---- the float64 sandwich -----------------------------------------------------------------------------------------------------------
def scale(rec, tris):
    q = triref.callers(rec)
    return 2.0 ** -24 * (float(np.abs(q[triref.walked(rec)]).max()) + float(np.abs(tris).max()))


def tolerance(rec, tris):
    return clc.TOL_K * scale(rec, tris)


def margins(rec, tris):
    """-> (pair keys caller << 32 | prim, G) of every pair of a walked caller triangle whose two bounding boxes come within a tolerance of
    each other (a pair with G > 0 crosses in exact arithmetic, so its boxes overlap: no other pair can be required, and none is listed)"""
    rec = np.asarray(rec, f32)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)
    tlo, thi = T.min(1), T.max(1)
    Q = triref.callers(rec).astype(np.float64)
    tol = tolerance(rec, tris)
    ks, gs = [], []
    for i in np.flatnonzero(triref.walked(rec)):
        near = np.flatnonzero(((tlo <= Q[i].max(0) + 2 * tol) & (thi >= Q[i].min(0) - 2 * tol)).all(1))
        if len(near):
            ks.append((np.int64(i) << 32) | near)
            gs.append(triref.margin64(rec, tris, np.full(len(near), i), near))
    return (np.concatenate(ks), np.concatenate(gs)) if ks else (np.zeros(0, np.int64), np.zeros(0))


def check_against_float64(rec, tris, res):
    """The issue's check: every pair with G > tol is listed, no pair with G < -tol is; returns (pairs inside the band that are listed,
    listed, the smallest K at which the sandwich would still hold)."""
    tol = tolerance(rec, tris)
    k, G = margins(rec, tris)
    have = keys(res)
    assert np.all(np.isin(have, k))                                       # nothing listed outside the candidates
    listed = np.isin(k, have)
    print("    margins of listed pairs: min %.3g; of unlisted candidate pairs: max %.3g; tol %.3g" %
          (G[listed].min() if listed.any() else np.nan, G[~listed].max() if (~listed).any() else np.nan, tol))
    assert np.all(listed[G > tol]), ("missing", k[(G > tol) & ~listed][:5])
    assert not np.any(listed[G < -tol]), ("phantom", k[(G < -tol) & listed][:5])
    wrong = np.concatenate([-G[listed & (G < 0)], G[~listed & (G > 0)], [0.0]])
    return int((listed & (np.abs(G) <= tol)).sum()), len(have), float(wrong.max()) / scale(rec, tris)


# ---- raw calls with a guard behind the entries --------------------------------------------------------------------------------------
def raw_search(rt, fn, head, rec, flags, capacity, null_entries=False, tail=()):
    """One call of a pt_tri_search* entry point with a guard pattern in every entry: `fn(*head, tris, n, flags, offsets, entries, capacity,
    *tail)`.  The entry buffer holds capacity + 8 records.  Returns (status, offsets, (capacity + 8, 4) uint32 records)."""
    n = len(rec)
    offsets = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    entries = rt._aligned_zeros((capacity + 8, 4), np.uint32)
    entries[...] = GUARD
    st = fn(*head, rec.ctypes.data_as(C.POINTER(rt.PtTri)), C.c_uint64(n), C.c_uint32(flags), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            None if null_entries else entries.ctypes.data_as(C.POINTER(rt.PtCross)), C.c_uint64(capacity), *tail)
    return st, offsets, entries


# ---- the exact cases of the issue, on the mesh triangle (0,0,0), (1,0,0), (0,1,0) ----------------------------------------------------
EXACT_TRI = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], f32)
_E = 2.0 ** -20
EXACT = [   # (caller triangle, listed, what its edges must look like)
    ([[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 0.5]], True, "one of each"),        # pierces the interior
    ([[0.5, -2, -2], [0.5, 4, -2], [0.5, 1, 4]], True, "mesh only"),                # pierced by the hypotenuse (and a leg)
    ([[0.25, 0.25, 0], [0.25, 0.25, 1], [1, 1, 1]], True, "any"),                   # touches the face at one vertex
    ([[1, 0, 0], [2, 0, 1], [2, 1, 1]], True, "any"),                               # touches vertex to vertex
    ([[0.25, 0.25, 0], [2, 0.25, 0], [0.25, 2, 0]], False, None),                   # coplanar, overlapping
    ([[0.25, 0.25, _E], [2, 0.25, _E], [0.25, 2, _E]], False, None),                # parallel, at z = 2^-20
    ([[0, 0, 0], [1, 0, 0], [0, 0, 1]], True, "any"),                               # shares an edge, out of plane
    ([[0.875, 0.875, -1], [0.875, 0.875, 1], [2, 2, 0.5]], False, None),            # disjoint, bounding boxes overlapping
]


def exact_tris(rt):
    return rt.pack_tris(np.array([e[0] for e in EXACT], np.float64))


def assert_exact(res):
    """the lists of exact_tris over a scene whose triangle 0 is EXACT_TRI and whose other triangles are out of reach"""
    off, ent = words(res)
    want = [triref.edges_exact(e[0], EXACT_TRI) for e in EXACT]
    assert [w != 0 for w in want] == [e[1] for e in EXACT], want
    assert np.diff(off).tolist() == [int(e[1]) for e in EXACT], np.diff(off)
    assert ent[:, 0].tolist() == [0] * len(ent) and ent[:, 1].tolist() == [w for w in want if w], (ent, want)
    for (_, listed, shape), w in zip(EXACT, want):
        if shape == "one of each":
            assert bin(w).count("1") == 2 and bin(w & 7).count("1") == 1, w
        elif shape == "mesh only":
            assert bin(w).count("1") == 2 and (w & 7) == 0 and (w & 16), w


# ---- the audit: a caller triangle through every aimed position of every triangle ------------------------------------------------------
AUDIT_EPS = 2.0                 # the reach of an audit triangle, in tolerances (box_cases.AUDIT_EPS)


def aimed_tris(rt, tris):
    """-> ((4 n, 12) PtTri records, the triangle each is aimed at): through each of the four aimed positions p of every triangle
    (treeaudit.aimed_rays) the caller triangle p + eps n, p - eps n, p + eps t, with n the triangle's unit normal and t the unit
    direction of its first edge: the edge from p + eps n to p - eps n crosses the plane at p, eps away from it on either side."""
    import treeaudit as ta
    rays = ta.aimed_rays(tris)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)[rays.tri]
    e1 = T[:, 1] - T[:, 0]
    c = np.cross(e1, T[:, 2] - T[:, 0])
    with np.errstate(all="ignore"):
        n = c / np.linalg.norm(c, axis=1)[:, None]
        t = e1 / np.linalg.norm(e1, axis=1)[:, None]
    n, t = np.where(np.isfinite(n), n, [0.0, 0.0, 1.0]), np.where(np.isfinite(t), t, [1.0, 0.0, 0.0])
    eps = AUDIT_EPS * clc.TOL_K * 2.0 ** -24 * (float(np.abs(rays.P).max()) + float(np.abs(tris).max()))
    return rt.pack_tris(np.stack([rays.P + eps * n, rays.P - eps * n, rays.P + eps * t], 1).astype(f32)), rays.tri
