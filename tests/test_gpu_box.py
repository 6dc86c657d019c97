"""Box-overlap queries on the GPU (pt_box_count / pt_box_search).  Every result is an integer, so every check is an
equality: of the persistent, the one-box-per-thread and the brute-force kernels with the host twin (tests/test_box_host.py pins that to a
float32 restatement, to brute force and to float64) -- counts, offsets, the entries' words including the zero reserved words, their ORDER,
and the counters of PT_BOX_STATS; of truncated results with the full one; of the counts with the offsets."""

import numpy as np
import pytest

import box_cases as bc
import crossing_cases as cc
from routecheck import run_case

pytestmark = pytest.mark.gpu

N_BOXES = 2048
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "deepcomb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def boxes_for(rt, name, tris, n=N_BOXES):
    boxes = bc.box_records(rt, tris, n=n)
    if name in ("comb", "deepcomb"):
        # every fourth box holds the whole comb (the deep one overruns the 64-entry cap); the last quarter lies beside it and meets nothing
        boxes[0::4] = bc.whole_scene_box(rt, tris)
        boxes[-(n // 4):, 0] += 5.0; boxes[-(n // 4):, 4] += 5.0
    return boxes


def raw_records(rt, ctx, boxes, flags):
    """pt_box_search_host into records that start as a guard: (offsets, the (total, 4) uint32 records as the library wrote them)"""
    st, off, _ = bc.raw_search(rt, rt.lib.pt_box_search_host, (ctx.h,), boxes, flags, 0, True)
    assert st == 0
    total = int(off[-1])
    st, off, ent = bc.raw_search(rt, rt.lib.pt_box_search_host, (ctx.h,), boxes, flags, total)
    assert st == 0 and np.all(ent[total:] == bc.GUARD)
    return off, ent[:total]


@pytest.mark.parametrize("name", SCENES)
def test_search_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = bc.install(rt, orc, gpu_ctx, name)
    boxes = boxes_for(rt, name, tris)
    want = rt.box_search_bvh4(tris, b4, boxes, stats=True)
    counts = np.diff(want[0].astype(np.int64)).astype(np.uint32)
    assert counts.max() >= 2 and (counts == 0).any()
    for simple in (False, True):
        got = gpu_ctx.box_search(boxes, simple=simple)
        assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.uint32
        bc.assert_same_lists(got, want, ordered=True)
        assert np.array_equal(gpu_ctx.box_count(boxes, simple=simple), counts)
        off, rec = raw_records(rt, gpu_ctx, boxes, rt.PT_BOX_SIMPLE_KERNEL if simple else 0)
        assert np.array_equal(off, want[0]) and np.array_equal(rec, bc.records_of(want))      # all four words: the reserved ones are 0
    got = gpu_ctx.box_search(boxes, stats=True)
    st = gpu_ctx.stats()
    bc.assert_same_lists(got, want, ordered=True)
    assert {k: st[k] for k in COUNTERS} == want[3], (st, want[3])
    assert (st["stack_drops"] > 0) == (name == "deepcomb")
    assert np.array_equal(gpu_ctx.box_count(boxes, stats=True), counts)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == want[3], (st, want[3])
    brute = rt.box_search_bvh4(tris, None, boxes, brute_force=True, stats=True)
    bc.assert_same_lists(gpu_ctx.box_search(boxes, brute_force=True), brute, ordered=True)
    bc.assert_same_lists(gpu_ctx.box_search(boxes, brute_force=True, stats=True), brute, ordered=True)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute[3], (st, brute[3])
    assert np.array_equal(gpu_ctx.box_count(boxes, brute_force=True), np.diff(brute[0].astype(np.int64)).astype(np.uint32))
    off, rec = raw_records(rt, gpu_ctx, boxes, rt.PT_BOX_BRUTE_FORCE)
    assert np.array_equal(off, brute[0]) and np.array_equal(rec, bc.records_of(brute))
    if name in ("deepcomb", "spoiled"):
        bc.assert_subset(want, brute)
    else:
        bc.assert_same_lists(want, brute, ordered=False)                 # completeness: nothing dropped, every triangle reachable


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = bc.install(rt, orc, gpu_ctx, "soup1k")
    boxes = bc.box_records(rt, tris, n=8400)[4200:4200 + n].copy()       # around triangle centroids (the second half): every list has entries
    want = rt.box_search_bvh4(tris, b4, boxes)
    assert len(want[0]) == n + 1 and int(want[0][-1]) >= n
    for simple in (False, True):
        bc.assert_same_lists(gpu_ctx.box_search(boxes, simple=simple), want, ordered=True)
        assert np.array_equal(gpu_ctx.box_count(boxes, simple=simple), np.diff(want[0].astype(np.int64)))
    empty = gpu_ctx.box_search(boxes[:0])                                # n = 0: offsets = [0], no kernel
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and gpu_ctx.box_count(boxes[:0]).size == 0


def test_long_and_empty_lists_in_one_wavefront(rt, orc, gpu_ctx):
    tris, b4 = bc.install(rt, orc, gpu_ctx, "dragon50k_l0")
    boxes = bc.box_records(rt, tris, n=512)
    boxes[0::64] = bc.whole_scene_box(rt, tris)                          # one per wavefront holds the whole scene: 50,000 entries
    boxes[1::8, 0] = np.nan; boxes[3::16, 5] = np.inf; boxes[5::16, 2] = -np.inf; boxes[7::16, 6] = np.nan      # not walked
    boxes[9::16, 1] = boxes[9::16, 5] + 1.0                              # lo > hi on one axis
    want = rt.box_search_bvh4(tris, b4, boxes, stats=True)
    counts = np.diff(want[0].astype(np.int64))
    assert want[3]["stack_drops"] == 0
    assert np.all(counts[0::64] == tris.size // 9) and tris.size // 9 > 1000 and not counts[1::8].any() and not counts[3::16].any() and not counts[5::16].any()
    assert not counts[7::16].any() and not counts[9::16].any()
    for kw in ({}, {"simple": True}, {"stats": True}):
        bc.assert_same_lists(gpu_ctx.box_search(boxes, **kw), want, ordered=True)
        assert np.array_equal(gpu_ctx.box_count(boxes, **kw), counts)
    assert gpu_ctx.stats()["rays_closest"] == len(boxes)
    some = boxes[:64]                                                     # one wavefront of the mix through brute force
    bc.assert_same_lists(gpu_ctx.box_search(some, brute_force=True), rt.box_search_bvh4(tris, None, some, brute_force=True), ordered=True)
    # the (lo, hi) form packs the same records
    bc.assert_same_lists(gpu_ctx.box_search(boxes[:, 0:3], boxes[:, 4:7]), want, ordered=True)


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_truncation_at_a_capacity_on_the_host_route(rt, orc, gpu_ctx, kernel):
    """pt_box_search_host: the staging and the copy back.  What the kernels themselves do with `capacity` is checked on the device route,
    with the guard in the memory they write: box_torch_cases.py::truncation_on_the_device_route."""
    tris, b4 = bc.install(rt, orc, gpu_ctx, "soup1k")
    boxes = bc.box_records(rt, tris, n=1000)
    flags = {"persistent": 0, "simple": rt.PT_BOX_SIMPLE_KERNEL, "brute": rt.PT_BOX_BRUTE_FORCE}[kernel]
    want = rt.box_search_bvh4(tris, b4 if kernel != "brute" else None, boxes, brute_force=kernel == "brute")
    total = bc.assert_truncation(lambda cap, null: bc.raw_search(rt, rt.lib.pt_box_search_host, (gpu_ctx.h,), boxes, flags, cap, null), int(want[0][-1]))
    st, off, ent = bc.raw_search(rt, rt.lib.pt_box_search_host, (gpu_ctx.h,), boxes, flags, total)
    assert st == 0 and np.array_equal(off, want[0]) and np.array_equal(ent[:total], bc.records_of(want))
    part = gpu_ctx.box_search(boxes, capacity=total - 5, simple=kernel == "simple", brute_force=kernel == "brute")
    assert np.array_equal(part[0], want[0]) and len(part[1]) == total - 5 and np.array_equal(part[1], want[1][:total - 5])


def test_exact_cases(rt, gpu_ctx):
    tris = np.concatenate([bc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    boxes = bc.exact_boxes(rt)
    for kw in ({}, {"simple": True}, {"brute_force": True}):
        res = gpu_ctx.box_search(boxes, **kw)
        bc.assert_exact(res)
        assert np.array_equal(gpu_ctx.box_count(boxes, **kw), np.diff(res[0].astype(np.int64)))


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "truncation_on_the_device_route", "no_host_synchronisation_with_a_capacity",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/box_torch_cases.py in a child process (torch is imported before the package there)."""
    run_case("box_torch_cases", case)
