"""Shared by the plane-cut tests (tests/test_cut_host.py, tests/test_cut_pins.py, tests/test_cut_binding.py, tests/test_gpu_cut.py,
tests/cut_torchroute_cases.py): the plane sets, the float64 sandwich around cutref's margin, the comparisons of four-word lists, the
exact cases and the raw calls (include/mi355pt.h pt_cut_search)."""
import ctypes as C

import numpy as np

import closest_cases as clc
import cutref
from box_cases import BAND_CAP, assert_subset as _assert_subset2, install, keys                # noqa: F401  (re-exported)
from radius_cases import GUARD, assert_truncation, extent, owner                                # noqa: F401

f32 = np.float32
N_PLANES, N_BESIDE = 500, 50
PLANE_SEED = 7
SHIFT = 0.002                   # a plane passes through the centroid of a random triangle moved by up to SHIFT x the extent per axis
W_LO, W_HI = 0.01, 0.1          # the window is a cube around that point, its half-size uniform in [W_LO, W_HI] x the extent
# The smallest K (in units of 2^-24 (max|vertex| sum|n_k| + |d|)) from which the float64 sandwich holds on the host twin, over the 24
# scene-tree pairs of test_cut_host.py: no listed pair has G < 0 and no unlisted candidate pair G > 0 beyond it.  TOL_K = 16 is what is
# asserted.  Measured: 0 -- the twin's classification agrees with float64 on every candidate pair.  Listed pairs inside the band
# |G| <= tol: 10 of 20,302 on each built tree of dragon50k (0.05 %), 12 of 20,831 on its refitted tree, none on tetra, box, cornell, soup1k
# and torus.
MEASURED_K = 0.0
# The largest |n.p - d| (float64) of a cut_segments end point over the plane sets of test_cut_host.py (unit normals, |coordinates| <= 4):
# 1.84e-7 (tetra; box 1.70e-7, cornell 1.83e-7, soup1k 9.1e-8, dragon50k 9.2e-8, torus 8.4e-8) -- what rounding t and the point's three
# coordinates to float32 moves it.  The bound asserted is 4 x the largest seen.
END_TOL = 4 * 1.84e-7


def plane_records(rt, tris, n=N_PLANES, beside=N_BESIDE, seed=PLANE_SEED):
    """(n + beside, 12) PtCutPlane records.  The first n: a random unit normal (rounded to f32), through the centroid of a random mesh
    triangle moved by up to SHIFT x the extent per axis, the window a cube of half-size W_LO..W_HI x the extent around that point.  The
    last `beside`: the same construction moved 2 extents beside the scene along x, so their lists are empty.  Computed in float64, rounded
    to f32."""
    rng = np.random.default_rng(seed)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)
    ext = extent(tris)
    m = n + beside
    nrm = rng.normal(size=(m, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm = nrm.astype(f32)
    p = T[rng.integers(0, len(T), m)].mean(1) + (rng.random((m, 3)) * 2 - 1) * SHIFT * ext
    p[n:, 0] += 2.0 * ext + (T[..., 0].max() - T[..., 0].min())
    h = rng.uniform(W_LO, W_HI, m) * ext
    d = np.einsum("nc,nc->n", nrm.astype(np.float64), p)
    return rt.pack_cuts(nrm, d.astype(f32), (p - h[:, None]).astype(f32), (p + h[:, None]).astype(f32))


def scene_window(tris):
    """(lo, hi) of one window that holds the whole scene with room to spare"""
    v = np.asarray(tris, f32).reshape(-1, 3)
    return v.min(0) - f32(0.5), v.max(0) + f32(0.5)


def with_scene_window(rec, tris):
    """the same planes, each with the whole-scene window"""
    out = np.array(rec, f32)
    aligned = np.zeros((len(out) * 12 + 4,), f32)
    off = (-aligned.ctypes.data % 16) // 4
    res = aligned[off: off + len(out) * 12].reshape(-1, 12)
    res[...] = out
    res[:, 4:7], res[:, 8:11] = scene_window(tris)
    return res


def vertical_planes(rt, tris, n, seed=5):
    """n planes with the whole-scene window whose normals lie in the xy plane, through the middle of the scene: on the comb
    (scenes.comb_bvh4: every triangle spans the comb in x and y at its own z) each cuts every triangle, so every leaf passes the node
    test and the walk stacks as the box query's does"""
    v = np.asarray(tris, f32).reshape(-1, 3)
    mid = (v.min(0) + v.max(0)).astype(np.float64) * 0.5
    a = np.random.default_rng(seed).uniform(0.0, 2 * np.pi, n)
    nrm = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1).astype(f32)
    lo, hi = scene_window(tris)
    return rt.pack_cuts(nrm, (nrm.astype(np.float64) @ mid).astype(f32), lo, hi)


# ---- lists of four-word entries ------------------------------------------------------------------------------------------------------
def words(res):
    """(offsets, prim, code, t0, t1) -> (offsets as int64, (m, 4) uint32 entry words, t0 and t1 as their bits)"""
    offsets, prim, code, t0, t1 = res[:5]
    return np.asarray(offsets).astype(np.int64), np.stack([np.asarray(prim, np.uint32), np.asarray(code, np.uint32),
                                                            np.asarray(t0, f32).view(np.uint32), np.asarray(t1, f32).view(np.uint32)], axis=1)


def records_of(res):
    """the (m, 4) uint32 PtCut records of a result"""
    return words(res)[1]


def assert_same_lists(a, b, ordered):
    """Two results hold the same lists, entries word for word (t0 and t1 as bits): in the same order, or as sets (each list sorted by prim)."""
    (oa, ea), (ob, eb) = words(a), words(b)
    assert np.array_equal(oa, ob), np.flatnonzero(oa != ob)[:10]
    if not ordered:
        ea, eb = ea[np.lexsort((ea[:, 0], owner(oa)))], eb[np.lexsort((eb[:, 0], owner(ob)))]
    assert np.array_equal(ea, eb), np.flatnonzero((ea != eb).any(1))[:10]


def assert_subset(walk, brute):
    """Every entry of `walk` is in `brute`'s list of the same plane, all four words; returns how many of brute's entries are missing."""
    missing = _assert_subset2(walk, brute)                               # prim and code
    kb = keys(brute)
    order = np.argsort(kb)
    pos = order[np.searchsorted(kb[order], keys(walk))]
    assert np.array_equal(words(brute)[1][pos], words(walk)[1])
    return missing


# ---- the float64 sandwich -----------------------------------------------------------------------------------------------------------
def scale(rec, tris):
    """per record: 2^-24 (max|vertex| sum|n_k| + |d|)"""
    r = np.asarray(rec, f32).astype(np.float64)
    return 2.0 ** -24 * (float(np.abs(np.asarray(tris, f32)).max()) * np.abs(r[:, 0:3]).sum(1) + np.abs(r[:, 3]))


def candidates(rec, tris, chunk_pairs=1 << 21):
    """-> (pi, ti) of every pair of a walked record whose triangle passes stage (a) against the window: the f32 comparisons of the twin
    itself (cutref.box_stage), which no rounding of the plane test touches.  No other pair can be listed."""
    r = np.asarray(rec, f32)
    m = np.asarray(tris).size // 9
    sel_all = np.flatnonzero(cutref.walked(r))
    step = max(1, chunk_pairs // max(m, 1))
    ps, ts = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for s in range(0, len(sel_all), step):
        sel = sel_all[s:s + step]
        pi = np.repeat(sel, m); ti = np.tile(np.arange(m), len(sel))
        v0, e1, e2 = cutref.records(tris, ti)
        with np.errstate(all="ignore"):
            a = cutref.box_stage(r[pi], v0, v0 + e1, v0 + e2)
        ps.append(pi[a]); ts.append(ti[a])
    return np.concatenate(ps), np.concatenate(ts)


def check_against_float64(rec, tris, res):
    """The issue's check over the candidate pairs: every pair that straddles the plane by more than tol (G > tol) is listed, none that
    fails to straddle it by more than tol (G < -tol) is.  Returns (listed pairs inside the band, listed, the smallest K at which the
    sandwich would still hold, the planes with a candidate pair inside the band)."""
    pi, ti = candidates(rec, tris)
    G = cutref.margin64(rec, tris, pi, ti)
    unit = scale(rec, tris)[pi]
    tol = clc.TOL_K * unit
    k = (pi.astype(np.int64) << 32) | ti
    have = keys(res)
    assert np.all(np.isin(have, k))                                       # nothing listed outside the candidates
    listed = np.isin(k, have)
    print("    margins of listed pairs: min %.3g; of unlisted candidate pairs: max %.3g; tol about %.3g" %
          (G[listed].min() if listed.any() else np.nan, G[~listed].max() if (~listed).any() else np.nan, float(np.median(tol)) if len(tol) else np.nan))
    assert np.all(listed[G > tol]), ("missing", k[(G > tol) & ~listed][:5])
    assert not np.any(listed[G < -tol]), ("phantom", k[(G < -tol) & listed][:5])
    wrong = np.concatenate([(-G / unit)[listed & (G < 0)], (G / unit)[~listed & (G > 0)], [0.0]])
    in_band = np.abs(G) <= tol
    return int((listed & in_band).sum()), len(have), float(wrong.max()), np.unique(pi[in_band])


# ---- raw calls with a guard behind the entries --------------------------------------------------------------------------------------
def raw_search(rt, fn, head, rec, flags, capacity, null_entries=False, tail=()):
    """One call of a pt_cut_search* entry point with a guard pattern in every entry: `fn(*head, planes, n, flags, offsets, entries,
    capacity, *tail)`.  The entry buffer holds capacity + 8 records.  Returns (status, offsets, (capacity + 8, 4) uint32 records)."""
    n = len(rec)
    offsets = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    entries = rt._aligned_zeros((capacity + 8, 4), np.uint32)
    entries[...] = GUARD
    st = fn(*head, rec.ctypes.data_as(C.POINTER(rt.PtCutPlane)), C.c_uint64(n), C.c_uint32(flags), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            None if null_entries else entries.ctypes.data_as(C.POINTER(rt.PtCut)), C.c_uint64(capacity), *tail)
    return st, offsets, entries


# ---- the exact cases of the issue, on the mesh triangle (0,0,0), (1,0,0), (0,1,0) ----------------------------------------------------
EXACT_TRI = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], f32)
_E = 2.0 ** -20
_WIN = ([-2, -2, -2], [2, 2, 2])
EXACT = [   # (normal, d, lo, hi, listed)
    ([1, 0, 0], 0.25) + _WIN + (True,),                # through the interior: two bits, t exact
    ([1, 2, 0], 0.5) + _WIN + (True,),                 # through the interior, both t dyadic: 1/2 on v0-v1, 1/4 on v0-v2
    ([1, -1, 0], 0.0) + _WIN + (True,),                # through v0, v1 above and v2 below
    ([1, 1, 0], 0.0) + _WIN + (False,),                # through v0, the others above: not listed
    ([-1, -1, 0], 0.0) + _WIN + (True,),               # through v0, the others below: listed, zero length, t = 1 on both
    ([0, 1, 0], 0.0) + _WIN + (False,),                # contains the edge v0-v1, v2 above: not listed
    ([0, -1, 0], 0.0) + _WIN + (True,),                # contains the edge v0-v1, v2 below: listed, the segment is that edge
    ([0, 0, 1], 0.0) + _WIN + (False,),                # coplanar: not listed
    ([0, 0, 1], _E) + _WIN + (False,),                 # parallel at 2^-20: not listed
    ([0, 0, -1], -_E) + _WIN + (False,),               # the same from the other side
    ([1, 0, 0], 0.25, [1.5, -2, -2], [2, 2, 2], False),        # cutting, but the window beside the triangle: not listed
    ([1, 0, 0], 0.25, [0.5, 0.5, 0], [0.5, 0.5, 0], True),     # a zero-extent window on the hypotenuse is valid
]


def exact_planes(rt):
    return rt.pack_cuts([e[0] for e in EXACT], [e[1] for e in EXACT], [e[2] for e in EXACT], [e[3] for e in EXACT])


def assert_exact(res):
    """the lists of exact_planes over a scene whose triangle 0 is EXACT_TRI and whose other triangles are out of reach"""
    off, ent = words(res)
    want = [cutref.cut_exact(e[0], e[1], EXACT_TRI) if e[4] else None for e in EXACT]
    for e in EXACT:                                                         # (the window decides the case before last alone)
        assert (cutref.cut_exact(e[0], e[1], EXACT_TRI) is not None) == (e[4] or e[2] != _WIN[0]), e
    assert np.diff(off).tolist() == [int(e[4]) for e in EXACT], np.diff(off)
    got = [w for w in want if w is not None]
    assert ent[:, 0].tolist() == [0] * len(ent) and ent[:, 1].tolist() == [w[0] for w in got], (ent, got)
    for row, w in zip(ent, got):
        assert bin(int(w[0]) & 7).count("1") == 2
        for bits, t in zip(row[2:4], w[1:3]):                               # every t of these cases is a dyadic rational: exact in f32
            assert float(np.uint32(bits).view(f32)) == float(t), (row, w)
    # by name: the interior cut, the zero-length segment and the edge
    assert got[0] == (3 | 16, 0.25, 0.25) and got[1][1:] == (0.5, 0.25)
    assert got[3] == (1 | 4 | 8, 1, 1)
    assert got[4] == (2 | 4 | 8 | 16, 1, 1)


# ---- the audit: a plane through every aimed position of every triangle ----------------------------------------------------------------
def aimed_planes(rt, tris):
    """-> ((4 n, 12) PtCutPlane records, the triangle each is aimed at): through each of the four aimed positions p of every triangle
    (treeaudit.aimed_rays) the plane with the normal along the triangle's first edge, d = n.p, and the default window."""
    import treeaudit as ta
    rays = ta.aimed_rays(tris)
    T = np.asarray(tris, f32).reshape(-1, 3, 3).astype(np.float64)[rays.tri]
    e1 = T[:, 1] - T[:, 0]
    with np.errstate(all="ignore"):
        t = e1 / np.linalg.norm(e1, axis=1)[:, None]
    t = np.where(np.isfinite(t), t, [1.0, 0.0, 0.0]).astype(f32)
    d = np.einsum("nc,nc->n", t.astype(np.float64), rays.P)
    return rt.pack_cuts(t, d.astype(f32)), rays.tri
