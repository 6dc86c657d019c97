"""Hit lists on the CPU: the host twin pt_list_hits_bvh4 (include/mi355pt.h) against a float32 restatement of the
triangle test and of the result record over all triangles (tests/hitlistref.py), the tree walk against brute force (both on the twin), the
compositions with the crossing counts, the any-hit and the closest-hit walks, Moller-Trumbore in float64, the deck whose lists have a known
length and known distances, truncation at a capacity, and the error codes.  The GPU tests (tests/test_gpu_hitlist.py) pin the kernels to
this twin bit for bit.

Measured here (and written into DESIGN.md section 20), over crossing_cases.SCENES with ray_set(.., 2000, 11): pairs inside the band of
the float64 comparison: 12 of 12,445 listed pairs (tetra 0 of 2,089, box 2 of 2,342, cornell 2 of 1,780, soup1k 1 of 755, dragon50k 2 of
2,938, torus 5 of 2,541), none outside it disagrees; largest deviation of an agreed pair from float64: |dt| / max(1, t) 2.57e-6,
|du| 1.09e-4, |dv| 5.82e-5; deepest stack of the twin over the forests of these scenes 18 (dragon50k), 31 on the 4097-layer deck; no tree
of these scenes and no deck drops a push."""
import ctypes as C

import numpy as np
import pytest

import crossing_cases as cc
import crossref
import hitlist_cases as hc
import hitlistref

N_RAYS = 2000
RAY_SEED = 11


@pytest.fixture(scope="module")
def cases(rt):
    """name -> (triangles, rays, float32 restatement of the brute-force lists): computed once, never written to."""
    memo = {}

    def get(name):
        if name not in memo:
            tris = cc.geometry(rt, name)
            rays = cc.ray_set(rt, tris, N_RAYS, RAY_SEED)
            memo[name] = (tris, rays, hitlistref.brute_lists(rays, tris))
        return memo[name]
    return get


@pytest.mark.parametrize("name", cc.SCENES)
def test_brute_force_twin_equals_the_float32_restatement(rt, cases, name):
    tris, rays, ref = cases(name)
    got = rt.list_hits_bvh4(tris, None, rays, brute_force=True, stats=True)
    hc.assert_same_lists(got, ref)                                          # every bit, in index order
    assert got[0].dtype == np.uint64 and int(ref[0][-1]) > 0
    assert np.array_equal(np.diff(ref[0].astype(np.int64)), crossref.crossings(rays, tris))
    assert got[5] == dict(rays_closest=len(rays), rays_shadow=0, nodes_examined=0, tris_tested=len(rays) * (tris.size // 9),
                          stack_drops=0, max_stack=0, samples=0)
    srt = rt.list_hits_bvh4(tris, None, rays, brute_force=True, sort=True)
    hc.assert_same_lists(srt, hitlistref.sort_lists(ref))
    hc.assert_sorted(srt)
    assert np.all(srt[1] > 0) and np.all(np.isfinite(srt[1]))               # bit order is value order


@pytest.mark.parametrize("name", cc.SCENES)
def test_walk_against_brute_force_on_every_tree(rt, orc, cases, name):
    base, _, _ = cases(name)
    deepest = 0
    for label, tris, b4 in cc.forest(rt, orc, base):
        rays = cc.ray_set(rt, tris, N_RAYS, RAY_SEED)
        brute = rt.list_hits_bvh4(tris, None, rays, brute_force=True, sort=True)
        walk = rt.list_hits_bvh4(tris, b4, rays, sort=True, stats=True)
        st = walk[5]
        assert st["stack_drops"] == 0 and st["rays_closest"] == len(rays) and 1 <= st["max_stack"] <= 64, (label, st)
        deepest = max(deepest, st["max_stack"])
        hc.assert_same_lists(walk, brute)                                   # nothing dropped: the sorted lists are equal, bit for bit
        # the unsorted list holds the same entries in visit order, and the counts are the crossing counts
        visit = rt.list_hits_bvh4(tris, b4, rays)
        hc.assert_same_lists(hitlistref.sort_lists(visit), brute)
        assert np.array_equal(np.diff(visit[0].astype(np.int64)), rt.count_hits_bvh4(tris, b4, rays))
    print("%s: deepest stack %d" % (name, deepest))


def test_comb_and_spoiled_list_a_subset(rt, orc):
    tris, b4 = cc.geometry(rt, "comb"), cc.comb_tree()
    rays = cc.comb_rays(rt, 512, 3)
    walk = rt.list_hits_bvh4(tris, b4, rays, stats=True)
    brute = rt.list_hits_bvh4(tris, None, rays, brute_force=True)
    assert walk[5]["stack_drops"] > 0 and walk[5]["max_stack"] == 64
    assert hc.rc.assert_subset(walk, brute) > 0                             # each triangle sits in one leaf; what is dropped is not listed
    # the compositions hold with drops too: the lengths are the crossing counts, a list is non-empty exactly when any-hit reports a hit
    counts = rt.count_hits_bvh4(tris, b4, rays)
    assert np.array_equal(np.diff(walk[0].astype(np.int64)), counts)
    hit = np.array([orc.trace_ray(tris, b4, r[0:3], r[4:7], anyhit=True)[0] for r in rays])
    assert np.array_equal(counts >= 1, hit) and hit.any()
    srt = rt.list_hits_bvh4(tris, b4, rays, sort=True)
    hc.assert_same_lists(srt, hitlistref.sort_lists(walk))

    tris = cc.geometry(rt, "spoiled")
    b4 = cc.spoiled_tree(rt, orc, tris)
    rays = cc.ray_set(rt, tris, N_RAYS, RAY_SEED)
    walk = rt.list_hits_bvh4(tris, b4, rays)
    brute = rt.list_hits_bvh4(tris, None, rays, brute_force=True)
    hc.rc.assert_subset(walk, brute)
    assert np.array_equal(np.diff(walk[0].astype(np.int64)), rt.count_hits_bvh4(tris, b4, rays))


@pytest.mark.parametrize("name", ["soup1k", "torus", "cornell"])
def test_compositions_with_any_hit_and_closest_hit(rt, orc, cases, name):
    tris, rays, _ = cases(name)
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    sub = rays[np.isinf(rays[:, 3])][:600]                                # orc_trace_ray has no t_max
    res = rt.list_hits_bvh4(tris, b4, sub, sort=True, stats=True)
    assert res[5]["stack_drops"] == 0
    off = res[0].astype(np.int64)
    assert np.array_equal(np.diff(off), rt.count_hits_bvh4(tris, b4, sub))
    any_hit = np.array([orc.trace_ray(tris, b4, r[0:3], r[4:7], anyhit=True)[0] for r in sub])
    assert np.array_equal(np.diff(off) >= 1, any_hit) and any_hit.any() and not any_hit.all()
    # the first sorted entry is the closest hit: t always; the triangle unless a second entry has the same t.  (The oracle reports t and
    # the triangle; u, v of an entry are pinned by the float32 restatement above.)
    ties = 0
    for i, r in enumerate(sub):
        hit, t, _, tri = orc.trace_ray(tris, b4, r[0:3], r[4:7])
        assert hit == (off[i + 1] > off[i])
        if hit:
            a = off[i]
            assert hc.bits(res[1][a:a + 1])[0] == hc.bits(np.float32([t]))[0], i
            tie = off[i + 1] - a > 1 and res[1][a + 1] == res[1][a]
            ties += int(tie)
            assert tie or res[2][a] == tri, i
    print("%s: %d closest hits with a second entry at the same t" % (name, ties))


def test_float64_semantics(rt, cases):
    dev = np.zeros(3)
    for name in cc.SCENES:
        tris, rays, _ = cases(name)
        got = rt.list_hits_bvh4(tris, None, rays, brute_force=True)
        off, ent = hc.words(got)
        n_tris = tris.size // 9
        listed = np.zeros((len(rays), n_tris), bool)
        own = hc.rc.owner(off)
        listed[own, ent[:, 1]] = True
        in_band = outside_bad = 0
        step = max(1, 2_000_000 // n_tris)
        for a in range(0, len(rays), step):
            hit, band, t, u, v = hitlistref.float64_pairs(rays[a:a + step], tris)
            part = listed[a:a + step]
            outside_bad += int(((hit != part) & ~band).sum())
            in_band += int((band & (hit | part)).sum())
            sel = (own >= a) & (own < a + step)
            ri, ti = own[sel] - a, ent[sel, 1]
            agreed = hit[ri, ti]
            tt = t[ri, ti][agreed]
            dev[0] = max(dev[0], np.max(np.abs(got[1][sel][agreed] - tt) / np.maximum(1, tt), initial=0))
            dev[1] = max(dev[1], np.max(np.abs(got[3][sel][agreed] - u[ri, ti][agreed]), initial=0))
            dev[2] = max(dev[2], np.max(np.abs(got[4][sel][agreed] - v[ri, ti][agreed]), initial=0))
        print("%s: %d of %d listed pairs in the band, %d disagreements outside it" % (name, in_band, len(ent), outside_bad))
        assert outside_bad == 0, name
        assert in_band * 100 <= len(ent), (name, in_band, len(ent))
    print("largest deviation from float64: |dt| / max(1, t) %.3g, |du| %.3g, |dv| %.3g" % tuple(dev))
    assert dev[0] <= hc.TOL_T and dev[1] <= hc.TOL_U and dev[2] <= hc.TOL_V, dev


@pytest.mark.parametrize("layers", hc.DECK_LAYERS)
def test_deck_lists_every_layer_in_order(rt, orc, layers):
    tris, z = hc.deck(layers, 7)
    b4 = cc.host_trees(rt, orc, tris, 0)[1]
    rays = hc.deck_rays(rt, 16, 3)
    res = rt.list_hits_bvh4(tris, b4, rays, sort=True, stats=True)
    assert res[5]["stack_drops"] == 0, res[5]                             # no deck drops at level 0, the 4097-layer one included
    off = res[0].astype(np.int64)
    assert np.all(np.diff(off) == layers)
    want = hc.deck_distances(z)
    for i in range(len(rays)):
        t = res[1][off[i]:off[i + 1]].astype(np.float64)
        assert np.all(np.diff(t) > 0)                                     # strictly ascending
        assert np.all(np.abs(t - want) <= hc.TOL_T * np.maximum(1, want))
        assert np.array_equal(np.sort(res[2][off[i]:off[i + 1]] // 2), np.arange(layers))     # one triangle of every quad
    visit = rt.list_hits_bvh4(tris, b4, rays)
    if layers >= 31:
        assert np.any(np.diff(visit[1][off[0]:off[1]]) < 0)               # tree order is not t order
    hc.assert_same_lists(hitlistref.sort_lists(visit), res)
    hc.assert_same_lists(rt.list_hits_bvh4(tris, None, rays, brute_force=True, sort=True), res)


def test_truncation_at_a_capacity(rt, orc):
    # a deck under t_max values that give every sort class, so that lists of several entries straddle the capacities, then a soup
    tris, z = hc.deck(65, 7)
    dist = hc.deck_distances(z)
    lens = np.array([0, 1, 2, 5, 16, 17, 33, 65] * 4)
    t_max = np.where(lens < 65, np.append(dist, np.inf)[lens] - 0.01, np.inf).astype(np.float32)
    t_max[lens == 0] = 0.5
    sets = [(tris, hc.deck_rays(rt, len(lens), 5, t_max))]
    soup = cc.geometry(rt, "soup1k")
    sets.append((soup, cc.ray_set(rt, soup, 500, RAY_SEED)))
    for tris, rays in sets:
        tree = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
        tp = tris.ctypes.data_as(C.POINTER(C.c_float))
        full = rt.list_hits_bvh4(tris, tree, rays)
        total = int(full[0][-1])
        off = full[0].astype(np.int64)
        inner = [int(off[i] + 1) for i in range(len(off) - 1) if off[i + 1] - off[i] > 2][:3]      # capacities inside a list
        for bp, w, flags in ((tree.ctypes.data_as(C.POINTER(C.c_uint32)), tree.size, 0), (None, 0, rt.PT_HITS_BRUTE_FORCE)):
            head = (tp, C.c_uint32(tris.size // 9), bp, C.c_uint64(w))

            def search(cap, null, sort):
                return hc.raw_list(rt, rt.lib.pt_list_hits_bvh4, head, rays, flags | (rt.PT_HITS_SORTED if sort else 0), cap, null, (None,))
            got, straddles = hc.assert_truncation(search, total, [0, 1, total - 1, total, total + 7] + inner)
            assert got == total and straddles > 0
    # the binding: capacity given -> the first entries, offsets complete
    part = rt.list_hits_bvh4(tris, tree, rays, capacity=100)
    assert np.array_equal(part[0], full[0]) and len(part[2]) == 100
    assert all(np.array_equal(hc.bits(a), hc.bits(b[:100])) for a, b in zip(part[1:5], full[1:5]))


def test_arguments_and_rays_that_are_not_walked(rt, orc):
    lib = rt.lib
    tris = cc.geometry(rt, "box")
    b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
    o = np.zeros((8, 3), np.float32); d = np.tile(np.float32([0.3, 0.2, 1.0]), (8, 1))
    rays = rt.pack_rays(o, d, [np.inf, 2.0, 0.5, 0.0, -1.0, np.nan, np.inf, np.inf])
    rays[6, 1] = np.nan; rays[7, 5] = np.nan
    for tree in (b4, None):
        res = rt.list_hits_bvh4(tris, tree, rays, stats=True, brute_force=tree is None, sort=True)
        assert np.diff(res[0].astype(np.int64)).tolist() == [1, 1, 0, 0, 0, 0, 0, 0]      # the wall at z = 1 is at t = 1
        assert res[1].tolist() == [1.0, 1.0] and res[5]["rays_closest"] == 8
    # from outside a closed box a ray crosses two walls, the nearer first once sorted
    out = rt.pack_rays([[0.1, 0.2, 3.0]] * 2, [[0, 0, -1], [0, 0, 1]])
    res = rt.list_hits_bvh4(tris, b4, out, sort=True)
    assert res[0].tolist() == [0, 2, 2] and res[1].tolist() == [2.0, 4.0]
    # an empty batch: offsets = [0]; a leaf whose triangle index is out of range is skipped
    empty = rt.list_hits_bvh4(tris, b4, np.zeros((0, 8), np.float32))
    assert empty[0].tolist() == [0] and len(empty[2]) == 0
    fewer = tris[:9 * 10]                                                  # the tree still names triangles 10 and 11 (the front)
    assert rt.list_hits_bvh4(fewer, b4, rays[:1])[0].tolist() == [0, 0]

    tp, bp = tris.ctypes.data_as(C.POINTER(C.c_float)), b4.ctypes.data_as(C.POINTER(C.c_uint32))
    rp = out.ctypes.data_as(C.POINTER(rt.PtRay))
    raw = np.zeros(4, np.uint64); off = raw[:2]
    ent = rt._aligned_zeros((16, 4), np.uint32)
    op, ep = off.ctypes.data_as(C.POINTER(C.c_uint64)), ent.ctypes.data_as(C.POINTER(rt.PtHit))
    n12, w = C.c_uint32(12), C.c_uint64(b4.size)

    def search(tp=tp, bp=bp, w=w, rp=rp, n=1, flags=0, op=op, ep=ep, cap=16):
        return lib.pt_list_hits_bvh4(tp, n12, bp, w, rp, C.c_uint64(n), C.c_uint32(flags), op, ep, C.c_uint64(cap), None)
    assert search() == 0 and off.tolist() == [0, 2]
    assert search(ep=None, cap=0) == 0 and off.tolist() == [0, 2]
    assert search(bp=None, w=C.c_uint64(0), flags=rt.PT_HITS_BRUTE_FORCE | rt.PT_HITS_SORTED) == 0 and off.tolist() == [0, 2]
    assert search(flags=rt.PT_HITS_SIMPLE_KERNEL | rt.PT_HITS_STATS | rt.PT_HITS_SORTED) == 0
    assert search(rp=None, ep=None, n=0, cap=0) == 0 and off[0] == 0
    # what the twin refuses, in which order and words: test_twin_query_errors.py
    assert C.sizeof(rt.PtHit) == 16 and C.sizeof(rt.PtRay) == 32
