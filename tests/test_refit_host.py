"""Refit in place, host side (include/mi355pt.h: pt_refit_bvh4, pt_refit_bvh2, pt_bvh4_cost): the host twins of
pt_update_triangles reproduce built trees word for word from unchanged triangles, equal a numpy restatement of the rules on deformed
ones, are memoryless, and a refitted tree renders in the oracle exactly what a rebuilt tree renders."""
import ctypes as C

import numpy as np
import pytest

import orc as orc_mod
from refit_cases import LEAF, check_refit_invariants, host_trees, numpy_cost, numpy_refit_bvh4, wave
from scenes import random_soup
from test_accel_host import DEGENERATE, degenerate

SOUPS = [(3000, 11), (20000, 5)]
AMPS = (0.02, 0.1, 0.3)


def scene_of(rt, name):
    if name == "soup3000":
        return random_soup(3000, 11)
    if name == "soup20000":
        return random_soup(20000, 5)
    if name == "dragon20000":
        return rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    return degenerate(name)


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["soup3000", "soup20000", "dragon20000"] + DEGENERATE)
def test_unchanged_triangles_reproduce_the_built_tree(rt, orc, name, accel):
    tris = scene_of(rt, name)
    b2, b4 = host_trees(rt, orc, tris, accel)
    assert np.array_equal(rt.refit_bvh4(tris, b4), b4)
    assert np.array_equal(rt.refit_bvh2(tris, b2), b2)
    if accel == 0:
        ob2, ob4 = orc.build_bvh4(tris)
        assert np.array_equal(rt.refit_bvh4(tris, ob4), ob4) and np.array_equal(rt.refit_bvh2(tris, ob2), ob2)


@pytest.mark.parametrize("accel", [0, 1, 2])
@pytest.mark.parametrize("name", ["soup3000", "soup20000", "dragon20000", "coplanar", "mixed_zero", "signed_zero"])
def test_deformed_trees_equal_the_numpy_restatement(rt, orc, name, accel):
    tris = scene_of(rt, name)
    b2, b4 = host_trees(rt, orc, tris, accel)
    for amp, frame in ((0.02, 0), (0.1, 3), (0.3, 7)):
        moved = wave(tris, amp, frame)
        got = rt.refit_bvh4(moved, b4)
        assert np.array_equal(got, numpy_refit_bvh4(moved, b4)), (amp, frame)
        check_refit_invariants(b4, got)
        # BVH2: topology untouched, leaves by the leaf rule (the same words as the BVH4's leaves), internal boxes contain their children's
        got2 = rt.refit_bvh2(moved, b2)
        nn2 = int(b2[0])
        r2, o2 = got2[1:].reshape(nn2, 6), b2[1:].reshape(nn2, 6)
        assert np.array_equal(r2[:, 3:], o2[:, 3:])
        r4 = got[1:].reshape(-1, 8)
        l4 = (r4[:, 7] & LEAF) != 0
        l2 = (r2[:, 5] & LEAF) != 0
        by_tri4 = np.zeros((tris.size // 9, 3), np.uint32); by_tri4[r4[l4, 7] & 0x7FFFFFFF] = r4[l4, :3]
        assert np.array_equal(r2[l2, :3], by_tri4[r2[l2, 5] & 0x7FFFFFFF])


@pytest.mark.parametrize("n,seed", SOUPS)
def test_oracle_renders_of_refitted_and_rebuilt_trees_are_identical(rt, orc, n, seed):
    tris = random_soup(n, seed)
    _, b4 = orc.build_bvh4(tris)
    w, h = 96, 64
    for amp in AMPS:
        moved = wave(tris, amp, 0)
        refit = rt.refit_bvh4(moved, b4)
        _, rebuilt = orc.build_bvh4(moved)
        p = orc.make_params(w, h, n, (0, 0, 2.5), (0, 0, 0, 1), mode=orc_mod.MODE_SINGLE)
        a, _, sa = orc.render(p, moved, refit)
        b, _, sb = orc.render(p, moved, rebuilt)
        differing = int(np.any(a.view(np.uint32) != b.view(np.uint32), -1).sum())
        print("n=%d amp=%.2f differing pixels %d, nodes_examined x%.3f" % (n, amp, differing, sa["nodes_examined"] / sb["nodes_examined"]))
        assert differing == 0
        assert sa["stack_drops"] == 0 and sb["stack_drops"] == 0


@pytest.mark.parametrize("accel", [0, 2])
def test_refit_is_memoryless(rt, orc, accel):
    tris = random_soup(3000, 11)
    b2, b4 = host_trees(rt, orc, tris, accel)
    cur4, cur2 = b4, b2
    for k in range(8):
        moved = wave(tris, 0.05 * (k + 1), k)
        cur4, cur2 = rt.refit_bvh4(moved, cur4), rt.refit_bvh2(moved, cur2)
    assert np.array_equal(cur4, rt.refit_bvh4(moved, b4)) and np.array_equal(cur2, rt.refit_bvh2(moved, b2))
    assert np.array_equal(rt.refit_bvh4(tris, cur4), b4) and np.array_equal(rt.refit_bvh2(tris, cur2), b2)


@pytest.mark.parametrize("n,seed", SOUPS)
def test_cost_against_numpy_and_grows_with_the_deformation(rt, orc, n, seed):
    tris = random_soup(n, seed)
    _, b4 = orc.build_bvh4(tris)
    m = int(b4[0])

    def cost(tree):
        got, want = rt.bvh4_cost(tree), numpy_cost(tree)
        print("cost", got, "numpy", want)
        assert abs(got - want) <= m * 2.0 ** -51 * want
        return got
    at_build = cost(b4)
    refit = {amp: cost(rt.refit_bvh4(wave(tris, amp, 0), b4)) for amp in AMPS}
    rebuilt = {amp: cost(orc.build_bvh4(wave(tris, amp, 0))[1]) for amp in AMPS}
    assert refit[0.3] > at_build
    assert refit[0.1] > rebuilt[0.1] and refit[0.3] > rebuilt[0.3]


def test_cost_of_leaf_roots_empty_and_installed_trees(rt, orc):
    one = random_soup(1, 0)
    assert rt.bvh4_cost(orc.build_bvh4(one)[1]) == 0.0                    # the root is a leaf
    assert rt.bvh4_cost(np.zeros(1, np.uint32)) == 0.0
    tris = random_soup(500, 9)
    b2, _ = orc.build_bvh4(tris)
    wide = rt.bvh2_to_bvh4_wide(b2)                                       # holds BVH2 nodes that no path from the root reaches
    assert abs(rt.bvh4_cost(wide) - numpy_cost(wide)) <= int(wide[0]) * 2.0 ** -51 * numpy_cost(wide)
    moved = rt.refit_bvh4(wave(tris, 0.1, 1), wide)                      # only what the root reaches is refitted; the topology stays
    assert np.array_equal(moved[1:].reshape(-1, 8)[:, 3:], wide[1:].reshape(-1, 8)[:, 3:]) and not np.array_equal(moved, wide)
    assert abs(rt.bvh4_cost(moved) - numpy_cost(moved)) <= int(wide[0]) * 2.0 ** -51 * numpy_cost(moved)
    spoiled = wide.copy(); spoiled[1:4] = (0x7C007C00, 0xFC007C00, 0xFC00FC00)     # a degenerate root
    assert rt.bvh4_cost(spoiled) == 0.0


def test_argument_errors_of_the_host_twins(rt, orc):
    tris = random_soup(50, 1)
    b2, b4 = orc.build_bvh4(tris)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    t = tris.ctypes.data_as(f32p)
    cost = C.c_double(-1.0)
    w4, w2 = b4.copy(), b2.copy()
    assert rt.lib.pt_refit_bvh4(t, 50, None, C.c_uint64(b4.size)) == 1                              # PT_ERR_INVALID_ARG
    assert rt.lib.pt_refit_bvh4(None, 50, w4.ctypes.data_as(u32p), C.c_uint64(b4.size)) == 1
    assert rt.lib.pt_refit_bvh2(t, 50, None, C.c_uint64(b2.size)) == 1
    assert rt.lib.pt_refit_bvh2(None, 50, w2.ctypes.data_as(u32p), C.c_uint64(b2.size)) == 1
    assert rt.lib.pt_bvh4_cost(None, C.c_uint64(b4.size), C.byref(cost)) == 1
    assert rt.lib.pt_bvh4_cost(w4.ctypes.data_as(u32p), C.c_uint64(b4.size), None) == 1
    assert rt.lib.pt_refit_bvh4(t, 50, w4.ctypes.data_as(u32p), C.c_uint64(b4.size - 1)) == 5       # PT_ERR_BAD_BVH: shorter than its node count
    assert rt.lib.pt_refit_bvh2(t, 50, w2.ctypes.data_as(u32p), C.c_uint64(b2.size - 1)) == 5
    assert rt.lib.pt_bvh4_cost(w4.ctypes.data_as(u32p), C.c_uint64(0), C.byref(cost)) == 5
    assert np.array_equal(w4, b4) and np.array_equal(w2, b2)                                        # nothing was written
    twice = b4.copy(); twice[1 + 3] = twice[1 + 4]                                                  # the root's first two slots name one child
    with pytest.raises(rt.PtError) as e:
        rt.refit_bvh4(tris, twice)
    assert e.value.code == 5
    assert rt.lib.pt_refit_bvh4(None, 0, w4.ctypes.data_as(u32p), C.c_uint64(b4.size)) == 0         # no triangles: every leaf keeps its words
    assert np.array_equal(w4[1:].reshape(-1, 8)[:, 3:], b4[1:].reshape(-1, 8)[:, 3:])
