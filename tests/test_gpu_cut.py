"""Plane-cut queries on the GPU (pt_cut_count / pt_cut_search).  Every result is an integer or a bit pattern, so
every check is an equality: of the persistent, the one-plane-per-thread and the brute-force kernels with the host twin
(tests/test_cut_host.py pins that to a float32 restatement, to brute force and to float64) -- counts, offsets, all four entry words with t0
and t1 as bits, their ORDER, and the counters of PT_CUT_STATS; of truncated results with the full one; of the counts with the offsets.
The torch-route cases are tests/cut_torchroute_cases.py, one child process each."""

import numpy as np
import pytest

import crossing_cases as cc
import cut_cases as ctc
from routecheck import run_case

pytestmark = pytest.mark.gpu

N_PLANES = 2048
SCENES = ["tetra", "torus", "soup1k", "dragon50k_l0", "dragon50k_l2", "refit", "bvh2", "comb", "deepcomb", "spoiled"]
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")


def planes_for(rt, name, tris, n=N_PLANES):
    rec = ctc.plane_records(rt, tris, n=n - n // 8, beside=n // 8)
    if name in ("comb", "deepcomb"):
        # every fourth plane holds the z direction and has the whole-scene window: it cuts every triangle of the comb (the deep one
        # overruns the 64-entry cap)
        rec[0::4] = ctc.vertical_planes(rt, tris, len(rec[0::4]))
    return rec


def raw_records(rt, ctx, rec, flags):
    """pt_cut_search_host into records that start as a guard: (offsets, the (total, 4) uint32 records as the library wrote them)"""
    st, off, _ = ctc.raw_search(rt, rt.lib.pt_cut_search_host, (ctx.h,), rec, flags, 0, True)
    assert st == 0
    total = int(off[-1])
    st, off, ent = ctc.raw_search(rt, rt.lib.pt_cut_search_host, (ctx.h,), rec, flags, total)
    assert st == 0 and np.all(ent[total:] == ctc.GUARD)
    return off, ent[:total]


@pytest.mark.parametrize("name", SCENES)
def test_search_equals_the_host_twin(rt, orc, gpu_ctx, name):
    tris, b4 = ctc.install(rt, orc, gpu_ctx, name)
    rec = planes_for(rt, name, tris)
    want = rt.cut_search_bvh4(tris, b4, rec, stats=True)
    counts = np.diff(want[0].astype(np.int64)).astype(np.uint32)
    assert counts.max() >= 1 and (counts == 0).any()
    for simple in (False, True):
        got = gpu_ctx.cut_search(rec, simple=simple)
        assert [x.dtype for x in got] == [np.uint64, np.uint32, np.uint32, np.float32, np.float32]
        ctc.assert_same_lists(got, want, ordered=True)
        assert np.array_equal(gpu_ctx.cut_count(rec, simple=simple), counts)
        off, ent = raw_records(rt, gpu_ctx, rec, rt.PT_CUT_SIMPLE_KERNEL if simple else 0)
        assert np.array_equal(off, want[0]) and np.array_equal(ent, ctc.records_of(want))     # all four words
    got = gpu_ctx.cut_search(rec, stats=True)
    st = gpu_ctx.stats()
    ctc.assert_same_lists(got, want, ordered=True)
    assert {k: st[k] for k in COUNTERS} == want[5], (st, want[5])
    assert (st["stack_drops"] > 0) == (name == "deepcomb")
    assert np.array_equal(gpu_ctx.cut_count(rec, stats=True), counts)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == want[5], (st, want[5])
    brute = rt.cut_search_bvh4(tris, None, rec, brute_force=True, stats=True)
    ctc.assert_same_lists(gpu_ctx.cut_search(rec, brute_force=True), brute, ordered=True)
    ctc.assert_same_lists(gpu_ctx.cut_search(rec, brute_force=True, stats=True), brute, ordered=True)
    st = gpu_ctx.stats()
    assert {k: st[k] for k in COUNTERS} == brute[5], (st, brute[5])
    assert np.array_equal(gpu_ctx.cut_count(rec, brute_force=True), np.diff(brute[0].astype(np.int64)).astype(np.uint32))
    off, ent = raw_records(rt, gpu_ctx, rec, rt.PT_CUT_BRUTE_FORCE)
    assert np.array_equal(off, brute[0]) and np.array_equal(ent, ctc.records_of(brute))
    if name in ("deepcomb", "spoiled"):
        ctc.assert_subset(want, brute)
    else:
        ctc.assert_same_lists(want, brute, ordered=False)                # completeness: nothing dropped, every triangle reachable


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes_at_the_chunk_edges(rt, orc, gpu_ctx, n):
    tris, b4 = ctc.install(rt, orc, gpu_ctx, "soup1k")
    rec = ctc.plane_records(rt, tris, n=8400, beside=0)[4200:4200 + n].copy()
    want = rt.cut_search_bvh4(tris, b4, rec)
    assert len(want[0]) == n + 1 and (n == 1 or int(want[0][-1]) >= 1)
    for simple in (False, True):
        ctc.assert_same_lists(gpu_ctx.cut_search(rec, simple=simple), want, ordered=True)
        assert np.array_equal(gpu_ctx.cut_count(rec, simple=simple), np.diff(want[0].astype(np.int64)))
    empty = gpu_ctx.cut_search(rec[:0])                                  # n = 0: offsets = [0], no kernel
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and gpu_ctx.cut_count(rec[:0]).size == 0


def test_long_and_empty_lists_in_one_wavefront(rt, orc, gpu_ctx):
    tris, b4 = ctc.install(rt, orc, gpu_ctx, "dragon50k_l0")
    rec = ctc.plane_records(rt, tris, n=512, beside=0)
    rec[0::64] = ctc.with_scene_window(rec[0::64], tris)                 # one per wavefront has the whole-scene window
    rec[1::8, 0] = np.nan; rec[3::16, 3] = np.inf; rec[5::16, 10] = -np.inf; rec[7::16, 0:3] = 0.0      # not walked
    rec[9::16, 4] = rec[9::16, 8] + np.float32(1.0)                      # lo > hi: not walked
    rec[11::16, 3] += np.float32(40.0)                                   # walked, the plane beside the scene: empty lists
    want = rt.cut_search_bvh4(tris, b4, rec, stats=True)
    counts = np.diff(want[0].astype(np.int64))
    assert want[5]["stack_drops"] == 0
    assert np.all(counts[0::64] > 200) and not counts[1::8].any() and not counts[3::16].any() and not counts[5::16].any()
    assert not counts[7::16].any() and not counts[9::16].any() and not counts[11::16].any()
    for kw in ({}, {"simple": True}, {"stats": True}):
        ctc.assert_same_lists(gpu_ctx.cut_search(rec, **kw), want, ordered=True)
        assert np.array_equal(gpu_ctx.cut_count(rec, **kw), counts)
    assert gpu_ctx.stats()["rays_closest"] == len(rec)
    some = rec[:64]                                                       # one wavefront of the mix through brute force
    ctc.assert_same_lists(gpu_ctx.cut_search(some, brute_force=True), rt.cut_search_bvh4(tris, None, some, brute_force=True), ordered=True)
    # the split form packs the same records
    ctc.assert_same_lists(gpu_ctx.cut_search(rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 8:11]), want, ordered=True)
    # cross_section: one call, every cut triangle once, the brute-force set
    nrm, d = rec[0, 0:3], rec[0, 3]
    prim, code, seg = gpu_ctx.cross_section(tris, nrm, d, grid=3)
    full = rt.cut_search_bvh4(tris, None, nrm, d, brute_force=True)
    assert len(np.unique(prim)) == len(prim) and np.array_equal(np.sort(prim), np.sort(full[1])) and seg.shape == (len(prim), 2, 3)


@pytest.mark.parametrize("kernel", ["persistent", "simple", "brute"])
def test_truncation_at_a_capacity_on_the_host_route(rt, orc, gpu_ctx, kernel):
    """pt_cut_search_host: the staging and the copy back.  What the kernels themselves do with `capacity` is checked on the device route,
    with the guard in the memory they write: cut_torchroute_cases.py::truncation_on_the_device_route."""
    tris, b4 = ctc.install(rt, orc, gpu_ctx, "soup1k")
    rec = ctc.plane_records(rt, tris, n=1000)
    flags = {"persistent": 0, "simple": rt.PT_CUT_SIMPLE_KERNEL, "brute": rt.PT_CUT_BRUTE_FORCE}[kernel]
    want = rt.cut_search_bvh4(tris, b4 if kernel != "brute" else None, rec, brute_force=kernel == "brute")
    total = ctc.assert_truncation(lambda cap, null: ctc.raw_search(rt, rt.lib.pt_cut_search_host, (gpu_ctx.h,), rec, flags, cap, null), int(want[0][-1]))
    st, off, ent = ctc.raw_search(rt, rt.lib.pt_cut_search_host, (gpu_ctx.h,), rec, flags, total)
    assert st == 0 and np.array_equal(off, want[0]) and np.array_equal(ent[:total], ctc.records_of(want))
    part = gpu_ctx.cut_search(rec, capacity=total - 5, simple=kernel == "simple", brute_force=kernel == "brute")
    assert np.array_equal(part[0], want[0]) and len(part[1]) == total - 5
    assert all(np.array_equal(p.view(np.uint32), w[:total - 5].view(np.uint32)) for p, w in zip(part[1:], want[1:5]))


def test_exact_cases(rt, gpu_ctx):
    tris = np.concatenate([ctc.EXACT_TRI, cc.geometry(rt, "box") + np.float32(4.0)])
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    rec = ctc.exact_planes(rt)
    for kw in ({}, {"simple": True}, {"brute_force": True}):
        res = gpu_ctx.cut_search(rec, **kw)
        ctc.assert_exact(res)
        assert np.array_equal(gpu_ctx.cut_count(rec, **kw), np.diff(res[0].astype(np.int64)))


@pytest.mark.parametrize("case", ["torch_route_equals_the_host_route", "truncation_on_the_device_route", "no_host_synchronisation_with_a_capacity",
                                  "ordering_with_batched_frames_and_scene_changes", "errors"])
def test_torch_route(case):
    """The device route: tests/cut_torchroute_cases.py in a child process (torch is imported before the package there)."""
    run_case("cut_torchroute_cases", case)
