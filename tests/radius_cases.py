"""Shared by the radius-query tests (tests/test_radius_host.py, tests/test_gpu_radius.py, tests/radius_torch_cases.py): the point sets with
their radii, the numpy restatement of the brute-force list, and the comparisons of lists (include/mi355pt.h pt_radius_search, DESIGN.md
section 18)."""
import ctypes as C

import numpy as np

import closest_cases as clc
import crossing_cases as cc
from refit_cases import wave
from scenes import random_soup

f32 = np.float32
N_POINTS = 500
POINT_SEED = 17
R_LO, R_HI = 0.01, 0.1          # radii are drawn continuously from [R_LO, R_HI] x the scene extent
# Per-scene upper radius factor where R_HI made the twin drop pushes at the 64-entry cap (none did: measured on the CPU over every scene of
# crossing_cases.SCENES and every tree of crossing_cases.forest, stack_drops = 0 throughout; DESIGN.md section 18 has the depths).
R_HI_OF = {}
WHOLE = 4.0                     # the whole-scene radius, in scene extents
GUARD = 0xA5A5A5A5


def install(rt, orc, ctx, name):
    """Sets the scene `name` on the context; returns (triangles, the BVH4 the context holds: what the host twin walks)."""
    if name == "comb":
        tris = cc.geometry(rt, "comb")
        ctx.set_triangles(tris); ctx.set_bvh4(cc.comb_tree())
    elif name == "spoiled":
        tris = cc.geometry(rt, "spoiled")
        ctx.set_triangles(tris); ctx.set_bvh4(cc.spoiled_tree(rt, orc, tris))
    elif name == "bvh2":
        tris = random_soup(2000, 31)
        ctx.set_triangles(tris); ctx.set_bvh2(orc.build_bvh4(tris)[0])
    elif name == "refit":
        base = cc.geometry(rt, "soup1k")
        ctx.set_triangles(base); ctx.build_bvh(1)
        tris = wave(base, 0.02, 3)
        ctx.update_triangles(tris)
    else:
        tris = cc.geometry(rt, name.split("_")[0])
        ctx.set_triangles(tris); ctx.build_bvh(2 if name.endswith("_l2") else 0)
    return tris, ctx.read_bvh4()


def extent(tris):
    v = np.asarray(tris, f32).reshape(-1, 3)
    return float((v.max(0) - v.min(0)).max())


def point_records(rt, tris, name=None, n=N_POINTS, seed=POINT_SEED):
    """(n, 4) PtPoint records: closest_cases.query_points with one radius each, uniform in [R_LO, R_HI] x the extent."""
    pts = clc.query_points(tris, n, seed)
    r = np.random.default_rng(seed + 1).uniform(R_LO, R_HI_OF.get(name, R_HI), n) * extent(tris)
    return rt.pack_points(pts, r.astype(f32))


def near_points(rt, tris, n, r_max, seed=POINT_SEED):
    """n points of the first quarter of query_points (uniform in 1.5 x the scene box) with one common r_max."""
    return rt.pack_points(clc.query_points(tris, 4 * n, seed)[:n], r_max)


def words(res):
    """(offsets, dist, prim, u, v) -> (offsets as int64, (m, 4) uint32 entry records)"""
    offsets, dist, prim, u, v = res[:5]
    e = np.stack([clc.bits(dist), np.asarray(prim, np.uint32), clc.bits(u), clc.bits(v)], axis=1) if len(prim) else np.zeros((0, 4), np.uint32)
    return np.asarray(offsets).astype(np.int64), e


def owner(offsets):
    """the point index of every entry"""
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def by_prim(offsets, entries):
    """the entries reordered so that every point's list is sorted by prim"""
    return entries[np.lexsort((entries[:, 1], owner(offsets)))]


def assert_same_lists(a, b, ordered):
    """Two results hold the same lists, entries bit for bit: in the same order, or as sets (each list sorted by prim)."""
    (oa, ea), (ob, eb) = words(a), words(b)
    assert np.array_equal(oa, ob), np.flatnonzero(oa != ob)[:10]
    if not ordered:
        ea, eb = by_prim(oa, ea), by_prim(ob, eb)
    assert np.array_equal(ea, eb), np.flatnonzero((ea != eb).any(1))[:10]


def assert_subset(walk, brute):
    """Every entry of `walk` is in `brute`'s list of the same point, bit for bit; returns how many of brute's entries are missing."""
    (ow, ew), (ob, eb) = words(walk), words(brute)
    kw = (owner(ow).astype(np.int64) << 32) | ew[:, 1]
    kb = (owner(ob).astype(np.int64) << 32) | eb[:, 1]
    assert len(np.unique(kw)) == len(kw)                                   # no triangle twice in a list
    order = np.argsort(kb)
    pos = np.searchsorted(kb[order], kw)
    assert np.all(pos < len(kb)) and np.array_equal(kb[order][np.minimum(pos, len(kb) - 1)], kw)
    assert np.array_equal(eb[order][pos], ew)
    return len(kb) - len(kw)


def numpy_brute(points, tris, chunk_pairs=1 << 20):
    """The brute-force list restated in numpy float32 (closest_cases.product_uv_d2 on every point-triangle pair): the triangles with
    d2 < r2 in index order, dist = sqrt(d2).  Returns (offsets, dist, prim, u, v)."""
    pts = np.asarray(points, f32)
    n, m = len(pts), np.asarray(tris).size // 9
    walked = ~np.isnan(pts).any(1) & (pts[:, 3] > 0)
    with np.errstate(over="ignore"):
        r2 = pts[:, 3] * pts[:, 3]
    counts = np.zeros(n, np.int64)
    cols = [[], [], [], []]
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
        counts += np.bincount(pi[keep], minlength=n)
        for c, a in zip(cols, (np.sqrt(d2[keep]), ti[keep].astype(np.uint32), u[keep], v[keep])):
            c.append(a)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    dist, prim, u, v = (np.concatenate(c) if c else np.zeros(0, t) for c, t in zip(cols, (f32, np.uint32, f32, f32)))
    return offsets, dist.astype(f32), prim.astype(np.uint32), u.astype(f32), v.astype(f32)


def raw_search(rt, fn, head, points, flags, capacity, null_entries=False, tail=()):
    """One call of a pt_radius_search* entry point with a guard pattern in every entry: `fn(*head, points, n, flags, offsets, entries,
    capacity, *tail)`.  The entry buffer holds capacity + 8 records.  Returns (status, offsets, (capacity + 8, 4) uint32 records)."""
    n = len(points)
    offsets = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    entries = rt._aligned_zeros((capacity + 8, 4), np.uint32)
    entries[...] = GUARD
    rc = fn(*head, points.ctypes.data_as(C.POINTER(rt.PtPoint)), C.c_uint64(n), C.c_uint32(flags), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
            None if null_entries else entries.ctypes.data_as(C.POINTER(rt.PtClosest)), C.c_uint64(capacity), *tail)
    return rc, offsets, entries


def assert_truncation(search, total_of):
    """The issue's four capacities through `search(capacity, null_entries) -> (status, offsets, guarded entries)`: offsets identical,
    entries below min(total, capacity) identical, the guard behind them untouched."""
    rc, off0, ent0 = search(0, True)
    assert rc == 0
    total = int(off0[-1])
    assert total == total_of and total > 8 and off0[0] == 0
    rc, _, full = search(total, False)
    assert rc == 0
    assert not np.any(np.all(full[:total] == GUARD, axis=1))
    for cap in (total - 1, total, total + 7):
        rc, off, ent = search(cap, False)
        assert rc == 0 and np.array_equal(off, off0), cap
        held = min(total, cap)
        assert np.array_equal(ent[:held], full[:held]), cap
        assert np.all(ent[held:] == GUARD), cap
    return total
