"""Triangle-overlap queries on the GPU (pt_tri_count / pt_tri_search).  Every result is an integer, so every check is
an equality: of the persistent, the one-triangle-per-thread and the brute-force kernels with the host twin (tests/test_tri_host.py pins that
to a float32 restatement, to brute force and to float64) -- counts, offsets, the entries' words including the zero reserved words, their
ORDER, and the counters of PT_TRI_STATS; of truncated results with the full one; of the counts with the offsets.  The torch-route cases
are tests/tri_torchroute_cases.py, one child process each."""

import numpy as np
import pytest

import crossing_cases as cc
import tri_cases as tc
from routecheck import run_case

pytestmark = pytest.mark.gpu

N_TRIS = 2048
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "deepcomb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def callers_for(rt, name, tris, n=N_TRIS):
    rec = tc.caller_records(rt, tris, n=n)
    if name in ("comb", "deepcomb"):
        # every fourth caller triangle spans the whole comb (the deep one overruns the 64-entry cap); the last quarter lies beside it
        rec[0::4] = tc.whole_scene_tri(rt, tris)
        rec[-(n // 4):, 0::4] += 50.0
    return rec


def raw_records(rt, ctx, rec, flags):
    """pt_tri_search_host into records that start as a guard: (offsets, the (total, 4) uint32 records as the library wrote them)"""
    st, off, _ = tc.raw_search(rt, rt.lib.pt_tri_search_host, (ctx.h,), rec, flags, 0, True)
    assert st == 0
    total = int(off[-1])
    st, off, ent = tc.raw_search(rt, rt.lib.pt_tri_search_host, (ctx.h,), rec, flags, total)
    assert st == 0 and np.all(ent[total:] == tc.GUARD)
    return off, ent[:total]


@pytest.mark.parametrize("name", SCENES)
def test_search_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = tc.install(rt, orc, gpu_ctx, name)
    rec = callers_for(rt, name, tris)
    want = rt.tri_search_bvh4(tris, b4, rec, stats=True)
    counts = np.diff(want[0].astype(np.int64)).astype(np.uint32)
    assert counts.max() >= 1 and (counts == 0).any()
    for simple in (False, True):
        got = gpu_ctx.tri_search(rec, simple=simple)
        assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
        tc.assert_same_lists(got, want, ordered=True)
        assert np.array_equal(gpu_ctx.tri_count(rec, simple=simple), counts)
        off, ent = raw_records(rt, gpu_ctx, rec, rt.PT_TRI_SIMPLE_KERNEL if simple else 0)
        assert np.array_equal(off, want[0]) and np.array_equal(ent, tc.records_of(want))      # all four words: the reserved ones are 0
    got = gpu_ctx.tri_search(rec, stats=True)
    st = gpu_ctx.stats()
    tc.assert_same_lists(got, want, ordered=True)
    assert {k: st[k] for k in COUNTERS} == want[3], (st, want[3])
    assert (st["stack_drops"] > 0) == (name == "deepcomb")
    assert np.array_equal(gpu_ctx.tri_count(rec, stats=True), counts)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == want[3], (st, want[3])
    brute = rt.tri_search_bvh4(tris, None, rec, brute_force=True, stats=True)
    tc.assert_same_lists(gpu_ctx.tri_search(rec, brute_force=True), brute, ordered=True)
    tc.assert_same_lists(gpu_ctx.tri_search(rec, brute_force=True, stats=True), brute, ordered=True)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute[3], (st, brute[3])
    assert np.array_equal(gpu_ctx.tri_count(rec, brute_force=True), np.diff(brute[0].astype(np.int64)).astype(np.uint32))
    off, ent = raw_records(rt, gpu_ctx, rec, rt.PT_TRI_BRUTE_FORCE)
    assert np.array_equal(off, brute[0]) and np.array_equal(ent, tc.records_of(brute))
    if name in ("deepcomb", "spoiled"):
        tc.assert_subset(want, brute)
    else:
        tc.assert_same_lists(want, brute, ordered=False)                 # completeness: nothing dropped, every triangle reachable
    pairs, edges = gpu_ctx.intersecting_pairs(rec)
    assert np.array_equal(pairs[:, 0], tc.owner(want[0].astype(np.int64))) and np.array_equal(pairs[:, 1], want[1]) and np.array_equal(edges, want[2])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = tc.install(rt, orc, gpu_ctx, "soup1k")
    rec = tc.caller_records(rt, tris, n=8400)[4200:4200 + n].copy()
    want = rt.tri_search_bvh4(tris, b4, rec)
    assert len(want[0]) == n + 1 and (n == 1 or int(want[0][-1]) >= 1)
    for simple in (False, True):
        tc.assert_same_lists(gpu_ctx.tri_search(rec, simple=simple), want, ordered=True)
        assert np.array_equal(gpu_ctx.tri_count(rec, simple=simple), np.diff(want[0].astype(np.int64)))
    empty = gpu_ctx.tri_search(rec[:0])                                  # n = 0: offsets = [0], no kernel
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and gpu_ctx.tri_count(rec[:0]).size == 0


def test_long_and_empty_lists_in_one_wavefront(rt, orc, gpu_ctx):
    tris, b4 = tc.install(rt, orc, gpu_ctx, "dragon50k_l0")
    rec = tc.caller_records(rt, tris, n=512)
    rec[0::64] = tc.whole_scene_tri(rt, tris)                            # one per wavefront spans the whole scene
    rec[1::8, 0] = np.nan; rec[3::16, 5] = np.inf; rec[5::16, 10] = -np.inf; rec[7::16, 6] = np.nan      # not walked
    rec[9::16, 0::4] += 40.0                                             # walked, beside the scene: empty lists
    want = rt.tri_search_bvh4(tris, b4, rec, stats=True)
    counts = np.diff(want[0].astype(np.int64))
    assert want[3]["stack_drops"] == 0
    assert np.all(counts[0::64] > 200) and not counts[1::8].any() and not counts[3::16].any() and not counts[5::16].any()
    assert not counts[7::16].any() and not counts[9::16].any()
    for kw in ({}, {"simple": True}, {"stats": True}):
        tc.assert_same_lists(gpu_ctx.tri_search(rec, **kw), want, ordered=True)
        assert np.array_equal(gpu_ctx.tri_count(rec, **kw), counts)
    assert gpu_ctx.stats()["rays_closest"] == len(rec)
    some = rec[:64]                                                       # one wavefront of the mix through brute force
    tc.assert_same_lists(gpu_ctx.tri_search(some, brute_force=True), rt.tri_search_bvh4(tris, None, some, brute_force=True), ordered=True)
    # the (n, 3, 3) and (n, 9) forms pack the same records
    verts = rec.reshape(-1, 3, 4)[:, :, :3]
    tc.assert_same_lists(gpu_ctx.tri_search(verts), want, ordered=True)
    tc.assert_same_lists(gpu_ctx.tri_search(verts.reshape(-1, 9)), want, ordered=True)


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_truncation_at_a_capacity_on_the_host_route(rt, orc, gpu_ctx, kernel):
    """pt_tri_search_host: the staging and the copy back.  What the kernels themselves do with `capacity` is checked on the device route,
    with the guard in the memory they write: tri_torchroute_cases.py::truncation_on_the_device_route."""
    tris, b4 = tc.install(rt, orc, gpu_ctx, "soup1k")
    rec = tc.caller_records(rt, tris, n=1000)
    flags = {"persistent": 0, "simple": rt.PT_TRI_SIMPLE_KERNEL, "brute": rt.PT_TRI_BRUTE_FORCE}[kernel]
    want = rt.tri_search_bvh4(tris, b4 if kernel != "brute" else None, rec, brute_force=kernel == "brute")
    total = tc.assert_truncation(lambda cap, null: tc.raw_search(rt, rt.lib.pt_tri_search_host, (gpu_ctx.h,), rec, flags, cap, null), int(want[0][-1]))
    st, off, ent = tc.raw_search(rt, rt.lib.pt_tri_search_host, (gpu_ctx.h,), rec, flags, total)
    assert st == 0 and np.array_equal(off, want[0]) and np.array_equal(ent[:total], tc.records_of(want))
    part = gpu_ctx.tri_search(rec, capacity=total - 5, simple=kernel == "simple", brute_force=kernel == "brute")
    assert np.array_equal(part[0], want[0]) and len(part[1]) == total - 5 and np.array_equal(part[1], want[1][:total - 5])
    walk = rt.tri_search_bvh4(tris, b4, rec)                              # intersecting_pairs has no flags: the persistent walk's order
    pairs, edges = gpu_ctx.intersecting_pairs(rec, capacity=total - 5)
    assert len(pairs) == total - 5 and np.array_equal(pairs[:, 0], tc.owner(walk[0].astype(np.int64))[:total - 5])
    assert np.array_equal(pairs[:, 1], walk[1][:total - 5]) and np.array_equal(edges, walk[2][:total - 5])


def test_exact_cases(rt, gpu_ctx):
    tris = np.concatenate([tc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    rec = tc.exact_tris(rt)
    for kw in ({}, {"simple": True}, {"brute_force": True}):
        res = gpu_ctx.tri_search(rec, **kw)
        tc.assert_exact(res)
        assert np.array_equal(gpu_ctx.tri_count(rec, **kw), np.diff(res[0].astype(np.int64)))


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "truncation_on_the_device_route", "no_host_synchronisation_with_a_capacity",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/tri_torchroute_cases.py in a child process (torch is imported before the package there)."""
    run_case("tri_torchroute_cases", case)
