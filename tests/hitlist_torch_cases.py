"""The torch-route cases of tests/test_gpu_hitlist.py, one child process each (tests/torchroute.py).  python tests/hitlist_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import crossing_cases as cc
import hitlist_cases as hc
from torchroute import N, bits


def scene(rt, ctx):
    tris = cc.torus()
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def to_host(res):
    """(offsets, t, prim, u, v) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(bits(x)[:m].view(t) for x, t in zip(res[1:], (np.float32, np.uint32, np.float32, np.float32)))


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
    """pt_list_hits itself, per kernel, unsorted and sorted, into guarded device tensors (torchroute.truncation_on_the_device_route): at
    the shared capacities, at 1 and at two inside a list."""
    tris = scene(rt, ctx)
    rays_h = cc.ray_set(rt, tris, N, 11)
    seen = tr.truncation_on_the_device_route(
        rt, ctx, rays_h, (0, rt.PT_HITS_SIMPLE_KERNEL, rt.PT_HITS_BRUTE_FORCE),
        lambda tree: hc.words(rt.list_hits_bvh4(tris, tree, rays_h, brute_force=tree is None)), ctx.list_hits_device, hc.GUARD,
        more_capacities=lambda off: [1] + [int(off[i] + 1) for i in range(N) if off[i + 1] - off[i] > 2][:2],
        variants=((0, None), (rt.PT_HITS_SORTED, hc.sorted_records)))
    for off, _, caps in seen:                             # some capacity cuts a list of more than one hit in two
        assert any(np.any((off[:-1] < cap) & (off[1:] > cap) & (off[1:] - off[:-1] > 1)) for cap in caps)
    want = seen[-1][1]
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.list_hits(torch.from_numpy(rays_h).cuda(), capacity=len(want) - 1, brute_force=True)
    assert len(res[2]) == len(want) - 1 and np.array_equal(bits(res[2]), want[:-1, 1])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    tris = scene(rt, ctx)
    rays_h = cc.ray_set(rt, tris, N, 11)
    rays = torch.from_numpy(rays_h).cuda()
    cap = int(rt.list_hits_bvh4(tris, ctx.read_bvh4(), rays_h)[0][-1])

    def sequence():
        return list(ctx.list_hits(rays, capacity=cap)) + list(ctx.list_hits(rays, capacity=cap, sort=True))
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    assert int(want[0][-1]) == cap > N
    res = tr.returns_before_the_stream(sequence)
    assert torch.equal(res[0], want[0]) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res[1:], want[1:]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    rays = cc.ray_set(rt, tris, N, 11)
    want = rt.list_hits_bvh4(tris, ctx.read_bvh4(), rays, sort=True)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.list_hits(torch.from_numpy(rays).cuda(), capacity=int(want[0][-1]), sort=True))
    hc.assert_same_lists(to_host(res), want)
    hc.assert_same_lists(ctx.list_hits(rays, sort=True), rt.list_hits_bvh4(other, ctx.read_bvh4(), rays, sort=True))


def errors(rt, ctx):
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); rays[:, 0] = 0.2; rays[:, 1] = 0.1; rays[:, 2] = 3.0; rays[:, 3] = float("inf"); rays[:, 6] = -1.0
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    rp, op, ep = rays.data_ptr(), off.data_ptr(), ent.data_ptr()
    hits = (ctx.list_hits_device, [rp, 1, op, ep, 16, 0], [
        (0, 0), (2, 0), (3, 0),                           # null (NULL hits only with capacity 0)
        (0, rp + 4), (2, op + 4), (3, ep + 8),            # rays and hits: 16-byte aligned, offsets: 8-byte aligned
        (5, 16), (1, 1 << 32)])                           # unknown flag, n > UINT32_MAX

    def deck():
        ctx.set_triangles(hc.deck(10, 7)[0]); ctx.build_bvh()
    tr.refusals(rt, ctx, [hits], deck, host=[lambda: ctx.list_hits(np.zeros((1, 8), np.float32))], cpu=[lambda: ctx.list_hits(torch.zeros((4, 8)))])
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
    tr.main(globals())
