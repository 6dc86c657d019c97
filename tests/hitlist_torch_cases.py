"""The torch-route cases of tests/test_gpu_hitlist.py, run in a child process each: torch is imported BEFORE the package there, so that
libmi355pt binds to torch's copy of the HIP runtime (as tests/radius_torch_cases.py does).  python tests/hitlist_torch_cases.py NAME"""
import os
import sys

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import crossing_cases as cc  # noqa: E402
import hitlist_cases as hc  # noqa: E402
from scenes import random_soup  # noqa: E402

N = 4097


def scene(rt, ctx):
    tris = cc.torus()
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def to_host(res):
    """(offsets, t, prim, u, v) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(x.cpu().view(torch.int32).numpy()[:m].view(t) for x, t in zip(res[1:], (np.float32, np.uint32, np.float32, np.float32)))


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    rays = cc.ray_set(rt, tris, N, 11)
    b4 = ctx.read_bvh4()
    want = rt.list_hits_bvh4(tris, b4, rays)
    want_sorted = rt.list_hits_bvh4(tris, b4, rays, sort=True)
    total = int(want[0][-1])
    assert total > N
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(rays).cuda()               # (n, 8) records, zero-copy
        sized = ctx.list_hits(rec)                        # capacity=None: one read of offsets[-1]
        roomy = ctx.list_hits(rec, capacity=total + 100, simple=True, sort=True)
        split = ctx.list_hits(rec[:, 0:3].contiguous(), rec[:, 4:7].contiguous(), t_max=rec[:, 3].contiguous(), capacity=total, sort=True)
        assert all(x.is_cuda for x in sized) and sized[0].dtype == torch.int64 and sized[2].dtype == torch.uint32
        assert len(sized[1]) == total and len(roomy[1]) == total + 100
        got = [to_host(sized), to_host(roomy), to_host(split)]
    hc.assert_same_lists(got[0], want)
    hc.assert_same_lists(got[1], want_sorted)
    hc.assert_same_lists(got[2], want_sorted)
    hc.assert_same_lists(ctx.list_hits(rays, sort=True), want_sorted)      # and the numpy route


def truncation_on_the_device_route(rt, ctx):
    """pt_list_hits itself, per kernel, unsorted and sorted, at the capacities 0 (NULL entries), 1, total - 1, total, total + 7 and two
    inside a list: the entries go into a device tensor of capacity + 8 records filled with a guard pattern, so a store at or beyond
    `capacity` lands where it is seen."""
    tris = scene(rt, ctx)
    rays_h = cc.ray_set(rt, tris, N, 11)
    rays = torch.from_numpy(rays_h).cuda()
    guard = np.uint32(hc.GUARD).astype(np.int32)
    for base, tree in ((0, ctx.read_bvh4()), (rt.PT_HITS_SIMPLE_KERNEL, ctx.read_bvh4()), (rt.PT_HITS_BRUTE_FORCE, None)):
        want_off, want = hc.words(rt.list_hits_bvh4(tris, tree, rays_h, brute_force=tree is None))
        total = int(want_off[-1])
        assert total > N
        inner = [int(want_off[i] + 1) for i in range(N) if want_off[i + 1] - want_off[i] > 2][:2]
        straddles = 0
        for cap in [0, 1, total - 1, total, total + 7] + inner:
            for sort in (False, True):
                flags = base | (rt.PT_HITS_SORTED if sort else 0)
                off = torch.full((N + 1,), -1, dtype=torch.int64, device="cuda")
                ent = torch.full((cap + 8, 4), int(guard), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ctx.list_hits_device(rays.data_ptr(), N, off.data_ptr(), ent.data_ptr() if cap else 0, cap, flags)
                ctx.synchronize()
                got = ent.cpu().numpy().view(np.uint32)
                held = min(total, cap)
                expect = hc.sorted_records(want_off, want[:held], held) if sort else want[:held]
                assert np.array_equal(off.cpu().numpy(), want_off), (flags, cap)                  # complete whatever the capacity
                assert np.array_equal(got[:held], expect), (flags, cap, np.flatnonzero((got[:held] != expect).any(1))[:8])
                assert np.all(got[held:] == hc.GUARD), (flags, cap, np.flatnonzero((got[held:] != hc.GUARD).any(1))[:8] + held)
            straddles += int(np.any((want_off[:-1] < cap) & (want_off[1:] > cap) & (want_off[1:] - want_off[:-1] > 1)))
        assert straddles > 0
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.list_hits(rays, capacity=total - 1, brute_force=True)
    assert len(res[2]) == total - 1 and np.array_equal(res[2].cpu().view(torch.int32).numpy().view(np.uint32), want[:total - 1, 1])


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    bvh4 = ctx.read_bvh4()
    rays = cc.ray_set(rt, tris, N, 11)
    want = rt.list_hits_bvh4(tris, bvh4, rays, sort=True)
    ctx.set_batch(8)
    for f in range(3):                                    # queued by pt_set_batch, not launched yet
        ctx.render(ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    res = ctx.list_hits(torch.from_numpy(rays).cuda(), capacity=int(want[0][-1]), sort=True)      # launches the three frames first, then the query
    other = random_soup(5000, 47)
    ctx.set_triangles(other); ctx.build_bvh()             # after the query: its results stay those of the first scene
    hc.assert_same_lists(to_host(res), want)
    hc.assert_same_lists(ctx.list_hits(rays, sort=True), rt.list_hits_bvh4(other, ctx.read_bvh4(), rays, sort=True))      # the next query sees the second


def errors(rt, ctx):
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); rays[:, 0] = 0.2; rays[:, 1] = 0.1; rays[:, 2] = 3.0; rays[:, 3] = float("inf"); rays[:, 6] = -1.0
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    rp, op, ep = rays.data_ptr(), off.data_ptr(), ent.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: ctx.list_hits_device(rp, 1, op, ep, 16)) == 4                     # no scene
    assert code(lambda: ctx.list_hits_device(rp + 4, 1, op, ep, 16)) == 1                 # the pointers are checked before the scene
    assert code(lambda: ctx.list_hits_device(rp, 1, op, ep, 16, flags=16)) == 1           # ... and the flags
    assert code(lambda: ctx.list_hits_device(rp, 1 << 32, op, ep, 16)) == 1               # ... and n > UINT32_MAX
    tris, z = hc.deck(10, 7)
    ctx.set_triangles(tris); ctx.build_bvh()
    assert code(lambda: ctx.list_hits_device(0, 1, op, ep, 16)) == 1                      # null
    assert code(lambda: ctx.list_hits_device(rp, 1, 0, ep, 16)) == 1
    assert code(lambda: ctx.list_hits_device(rp, 1, op, 0, 16)) == 1                      # NULL hits only with capacity 0
    assert code(lambda: ctx.list_hits_device(rp + 4, 1, op, ep, 16)) == 1                 # rays: 16-byte aligned
    assert code(lambda: ctx.list_hits_device(rp, 1, op + 4, ep, 16)) == 1                 # offsets: 8-byte aligned
    assert code(lambda: ctx.list_hits_device(rp, 1, op, ep + 8, 16)) == 1                 # hits: 16-byte aligned
    assert code(lambda: ctx.list_hits_device(rp, 1, op, ep, 16, flags=16)) == 1           # unknown flag
    assert code(lambda: ctx.list_hits_device(rp, 1 << 32, op, ep, 16)) == 1               # n > UINT32_MAX
    off.fill_(7); ent.fill_(7)
    torch.cuda.synchronize()
    ctx.list_hits_device(rp, 0, op, ep, 16)                                               # n = 0: offsets[0] = 0, nothing else
    ctx.list_hits_device(rp, 63, op + 8, 0, 0, flags=rt.PT_HITS_SORTED)                   # offsets only (64 words from off[1] on), at an 8-byte aligned address
    ctx.synchronize()
    assert int(off[0]) == 0 and int(ent.min()) == 7 and int(ent.max()) == 7
    assert int(off[1]) == 0 and int(off[2]) == 10 and int(off[64]) == 630                 # every ray crosses the ten layers
    t, prim = ctx.list_hits(np.float32([[0.2, 0.1, 3, np.inf, 0, 0, -1, 0]]), sort=True)[1:3]      # the context is still usable
    assert len(prim) == 10 and np.all(np.diff(t) > 0)


if __name__ == "__main__":
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
