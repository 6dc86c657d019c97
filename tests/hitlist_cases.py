"""Shared by the hit-list tests (tests/test_hitlist_host.py, tests/test_gpu_hitlist.py, tests/hitlist_torch_cases.py): the deck scene
whose lists have a known length and known distances, the comparisons of lists, and the truncation sweep (include/mi355pt.h pt_list_hits,
DESIGN.md section 20)."""
import ctypes as C

import numpy as np

import closest_cases as clc
import radius_cases as rc

f32 = np.float32
GUARD = rc.GUARD
LANE_MAX, LDS_MAX = 16, 512          # pt_kernels.h PT_HL_LANE_MAX, PT_HL_LDS_MAX: the class boundaries of hit_sort_kernel
# the issue's deck sizes and the lengths on both sides of each class boundary of the sort
DECK_LAYERS = [1, 2, LANE_MAX, LANE_MAX + 1, 31, 32, 33, 63, 64, 65, LDS_MAX, LDS_MAX + 1, 1000, 4097]
DECK_Z0, DECK_Z_LO, DECK_Z_HI = 3.0, -2.0, 2.0
# Deviation from float64 measured on the twin over crossing_cases.SCENES (tests/test_hitlist_host.py::test_float64_semantics, DESIGN.md
# section 20): |dt| / max(1, t) 2.6e-6, |du| 1.1e-4, |dv| 5.9e-5 (rounded up).  Asserted four times each: the
# margin covers other seeds, not other arithmetic.
DEV_T, DEV_U, DEV_V = 2.6e-6, 1.1e-4, 5.9e-5
TOL_T, TOL_U, TOL_V = 4 * DEV_T, 4 * DEV_U, 4 * DEV_V


def deck(layers, seed):
    """`layers` parallel unit quads (two triangles each, split along the diagonal x = y) at distinct z in [-2, 2], in shuffled order so
    that tree order is not t order.  Returns (triangles, z of quad k)."""
    rng = np.random.default_rng(seed)
    z = np.linspace(DECK_Z_LO, DECK_Z_HI, layers, dtype=np.float64).astype(f32) if layers > 1 else np.zeros(1, f32)
    assert len(np.unique(z)) == layers
    z = z[rng.permutation(layers)]
    a = np.stack([np.full(layers, -0.5, f32), np.full(layers, -0.5, f32), z], 1)
    b = np.stack([np.full(layers, 0.5, f32), np.full(layers, -0.5, f32), z], 1)
    c = np.stack([np.full(layers, 0.5, f32), np.full(layers, 0.5, f32), z], 1)
    d = np.stack([np.full(layers, -0.5, f32), np.full(layers, 0.5, f32), z], 1)
    tris = np.stack([a, b, c, a, c, d], 1).astype(f32).reshape(-1)
    return tris, z


def deck_rays(rt, n, seed, t_max=None):
    """n rays along -z from z = 3 through points at least 0.05 from every quad's border and diagonal."""
    rng = np.random.default_rng(seed)
    xy = np.zeros((0, 2))
    while len(xy) < n:
        p = rng.uniform(-0.45, 0.45, (4 * n + 16, 2))
        xy = np.concatenate([xy, p[np.abs(p[:, 0] - p[:, 1]) >= 0.05 * np.sqrt(2.0) + 1e-6]])
    xy = xy[:n]
    org = np.stack([xy[:, 0], xy[:, 1], np.full(n, DECK_Z0)], 1).astype(f32)
    return rt.pack_rays(org, np.tile(f32([0, 0, -1]), (n, 1)), t_max)


def deck_distances(z):
    """the known distances of a deck ray, ascending (float64)"""
    return np.sort(DECK_Z0 - np.asarray(z, np.float64))


def words(res):
    """(offsets, t, prim, u, v) -> (offsets as int64, (m, 4) uint32 entry records)"""
    return rc.words(res)


def assert_same_lists(a, b):
    """Two results hold the same lists in the same order, entries bit for bit."""
    rc.assert_same_lists(a, b, True)


def assert_sorted(res):
    """every list ascends in (t bits << 32 | prim)"""
    off, e = words(res)
    key = (e[:, 0].astype(np.uint64) << np.uint64(32)) | e[:, 1].astype(np.uint64)
    own = rc.owner(off)
    inside = own[1:] == own[:-1]
    assert np.all(key[1:][inside] >= key[:-1][inside])


def raw_list(rt, fn, head, rays, flags, capacity, null_entries=False, tail=()):
    """One call of a pt_list_hits* entry point with a guard pattern in every entry: `fn(*head, rays, n, flags, offsets, hits, capacity,
    *tail)`.  The entry buffer holds capacity + 8 records.  Returns (status, offsets, (capacity + 8, 4) uint32 records)."""
    n = len(rays)
    offsets = np.full(n + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)
    entries = rt._aligned_zeros((capacity + 8, 4), np.uint32)
    entries[...] = GUARD
    rc_ = fn(*head, rays.ctypes.data_as(C.POINTER(rt.PtRay)), C.c_uint64(n), C.c_uint32(flags), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
             None if null_entries else entries.ctypes.data_as(C.POINTER(rt.PtHit)), C.c_uint64(capacity), *tail)
    return rc_, offsets, entries


def sorted_records(off, ent, upto):
    """`ent` with every list that ends at or below `upto` sorted by the key (what PT_HITS_SORTED leaves of a visit-order buffer)"""
    out = ent.copy()
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        if b <= upto and b - a > 1:
            key = (out[a:b, 0].astype(np.uint64) << np.uint64(32)) | out[a:b, 1].astype(np.uint64)
            out[a:b] = out[a:b][np.argsort(key, kind="stable")]
    return out


def assert_truncation(search, total_of, capacities=None):
    """The capacities 0 (NULL entries), 1, total - 1, total and total + 7 through `search(capacity, null_entries, sort) -> (status,
    offsets, guarded entries)`: offsets identical; unsorted, the entries below min(total, capacity) are the visit-order prefix and the
    guard behind them is untouched; sorted, every fully stored list is the sorted visit-order list and the straddling list is the
    visit-order prefix."""
    rc_, off0, _ = search(0, True, False)
    assert rc_ == 0
    total = int(off0[-1])
    assert total == total_of and total > 8 and off0[0] == 0
    rc_, _, full = search(total, False, False)
    assert rc_ == 0
    assert not np.any(np.all(full[:total] == GUARD, axis=1))
    off = off0.astype(np.int64)
    straddles = 0
    for cap in capacities or (0, 1, total - 1, total, total + 7):
        for sort in (False, True):
            rc_, o, ent = search(cap, False, sort)
            assert rc_ == 0 and np.array_equal(o, off0), (cap, sort)
            held = min(total, cap)
            want = sorted_records(off, full[:held], held) if sort else full[:held]
            assert np.array_equal(ent[:held], want), (cap, sort, np.flatnonzero((ent[:held] != want).any(1))[:10])
            assert np.all(ent[held:] == GUARD), (cap, sort)
        straddles += int(np.any((off[:-1] < cap) & (off[1:] > cap) & (off[1:] - off[:-1] > 1)))
    return total, straddles


def bits(a):
    return clc.bits(a)
