"""Hit lists on the GPU (pt_list_hits).  Every result is an integer or a bit pattern, so every check is an equality:
of the persistent, the one-ray-per-thread and the brute-force kernels, unsorted and sorted, with the host twin (tests/test_hitlist_host.py
pins that to a float32 restatement, to brute force and to float64) -- offsets, the entries' bits and their ORDER, and the counters of
PT_HITS_STATS; of the list lengths with pt_count_hits; of the sort kernel's classes with the twin on a deck whose lists have every length
around the class boundaries; of truncated results with the full one."""

import numpy as np
import pytest

import crossing_cases as cc
import hitlist_cases as hc
import hitlistref
import radius_cases as rc
from radius_cases import install
from routecheck import run_case

pytestmark = pytest.mark.gpu

N_RAYS = 2048
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def rays_for(rt, name, tris, n=N_RAYS):
    return cc.comb_rays(rt, n, 3) if name == "comb" else cc.ray_set(rt, tris, n, 11)


@pytest.mark.parametrize("name", SCENES)
def test_every_kernel_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = install(rt, orc, gpu_ctx, name)
    rays = rays_for(rt, name, tris)
    want = rt.list_hits_bvh4(tris, b4, rays, stats=True)
    want_sorted = rt.list_hits_bvh4(tris, b4, rays, sort=True)
    counts = np.diff(want[0].astype(np.int64)).astype(np.uint32)
    assert counts.max() >= 2 and (name == "comb" or (counts == 0).any())
    for simple in (False, True):
        got = gpu_ctx.list_hits(rays, simple=simple)
        assert got[0].dtype == np.uint64 and got[2].dtype == np.uint32
        hc.assert_same_lists(got, want)
        hc.assert_same_lists(gpu_ctx.list_hits(rays, simple=simple, sort=True), want_sorted)
        assert np.array_equal(gpu_ctx.count_hits(rays, simple=simple), counts)
    for sort, w in ((False, want), (True, want_sorted)):
        hc.assert_same_lists(gpu_ctx.list_hits(rays, stats=True, sort=sort), w)
        st = gpu_ctx.stats()
        assert {k: st[k] for k in COUNTERS} == want[5], (st, want[5])
    assert (st["stack_drops"] > 0) == (name == "comb")
    brute = rt.list_hits_bvh4(tris, None, rays, brute_force=True, stats=True)
    brute_sorted = hitlistref.sort_lists(brute)
    hc.assert_same_lists(gpu_ctx.list_hits(rays, brute_force=True), brute)
    hc.assert_same_lists(gpu_ctx.list_hits(rays, brute_force=True, sort=True), brute_sorted)
    hc.assert_same_lists(gpu_ctx.list_hits(rays, brute_force=True, stats=True), brute)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute[5], (st, brute[5])
    assert np.array_equal(gpu_ctx.count_hits(rays, brute_force=True), np.diff(brute[0].astype(np.int64)).astype(np.uint32))
    if name in ("comb", "spoiled"):
        rc.assert_subset(want, brute)
    else:
        hc.assert_same_lists(want_sorted, brute_sorted)                  # nothing dropped, every triangle reachable: tree-independent


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = install(rt, orc, gpu_ctx, "torus")
    rays = cc.ray_set(rt, tris, 8400, 11)[1000:1000 + n].copy()
    want = rt.list_hits_bvh4(tris, b4, rays, sort=True)
    visit = rt.list_hits_bvh4(tris, b4, rays)
    assert len(want[0]) == n + 1
    for simple in (False, True):
        hc.assert_same_lists(gpu_ctx.list_hits(rays, simple=simple, sort=True), want)
        hc.assert_same_lists(gpu_ctx.list_hits(rays, simple=simple), visit)
    empty = gpu_ctx.list_hits(rays[:0], sort=True)                       # n = 0: offsets = [0], no kernel
    assert empty[0].tolist() == [0] and len(empty[2]) == 0


def mixed_deck_rays(rt, z):
    """256 rays over the 4097-layer deck: in every chunk of 64 every length of hitlist_cases.DECK_LAYERS (by t_max), rays that are not
    walked and rays that miss the deck."""
    dist = hc.deck_distances(z)
    lens = np.array((hc.DECK_LAYERS + [0, 3, 7, 10]) * 15)[:256]
    far = np.append(dist, np.inf)
    t_max = np.where(lens < len(dist), (far[np.maximum(lens, 1) - 1] + far[np.minimum(lens, len(dist) - 1)]) / 2, np.inf).astype(np.float32)
    t_max[lens == 0] = np.float32(dist[0] / 2)
    rays = hc.deck_rays(rt, 256, 5, t_max)
    rays[20::64, 3] = 0.0; rays[21::64, 3] = -1.0; rays[22::64, 3] = np.nan; rays[23::64, 4] = np.nan; rays[24::64, 1] = np.nan      # not walked
    rays[25::64, 0] = 2.0                                                                                                         # beside the deck
    lens = lens.copy()
    for k in range(20, 26):
        lens[k::64] = 0
    return rays, lens


def test_deck_exercises_every_sort_class_in_one_wavefront(rt, orc, gpu_ctx):
    tris, z = hc.deck(4097, 7)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(0)
    b4 = gpu_ctx.read_bvh4()
    rays, lens = mixed_deck_rays(rt, z)
    want = rt.list_hits_bvh4(tris, b4, rays, sort=True, stats=True)
    assert want[5]["stack_drops"] == 0
    assert np.array_equal(np.diff(want[0].astype(np.int64)), lens)        # every list has the length its t_max asks for
    assert set(hc.DECK_LAYERS) <= set(lens[:64].tolist())
    hc.assert_sorted(want)
    visit = rt.list_hits_bvh4(tris, b4, rays)
    assert not np.array_equal(hc.words(visit)[1], hc.words(want)[1])       # there was something to sort
    for simple in (False, True):
        hc.assert_same_lists(gpu_ctx.list_hits(rays, simple=simple, sort=True), want)
        hc.assert_same_lists(gpu_ctx.list_hits(rays, simple=simple), visit)
    hc.assert_same_lists(gpu_ctx.list_hits(rays, brute_force=True, sort=True), want)


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_truncation_at_a_capacity_on_the_host_route(rt, orc, gpu_ctx, kernel):
    """pt_list_hits_host: the staging and the copy back.  What the kernels themselves do with `capacity` is checked on the device route,
    with the guard in the memory they write: hitlist_torch_cases.py::truncation_on_the_device_route."""
    tris, b4 = install(rt, orc, gpu_ctx, "torus")
    rays = cc.ray_set(rt, tris, 1000, 11)
    flags = {"persistent": 0, "simple": rt.PT_HITS_SIMPLE_KERNEL, "brute": rt.PT_HITS_BRUTE_FORCE}[kernel]
    want = rt.list_hits_bvh4(tris, b4 if kernel != "brute" else None, rays, brute_force=kernel == "brute")
    off = want[0].astype(np.int64)
    inner = [int(off[i] + 1) for i in range(len(off) - 1) if off[i + 1] - off[i] > 2][:2]

    def search(cap, null, sort):
        return hc.raw_list(rt, rt.lib.pt_list_hits_host, (gpu_ctx.h,), rays, flags | (rt.PT_HITS_SORTED if sort else 0), cap, null)
    total, straddles = hc.assert_truncation(search, int(want[0][-1]), [0, 1, int(want[0][-1]) - 1, int(want[0][-1]), int(want[0][-1]) + 7] + inner)
    assert straddles > 0
    rc_, o, ent = search(total, False, False)
    assert rc_ == 0 and np.array_equal(o, want[0]) and np.array_equal(ent[:total], hc.words(want)[1])
    part = gpu_ctx.list_hits(rays, capacity=total - 5, simple=kernel == "simple", brute_force=kernel == "brute")
    assert np.array_equal(part[0], want[0]) and len(part[2]) == total - 5 and np.array_equal(part[2], want[2][:total - 5])


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "truncation_on_the_device_route", "no_host_synchronisation_with_a_capacity",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/hitlist_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("hitlist_torch_cases", case)
