"""The torch-route cases of tests/test_gpu_radius.py, one child process each (tests/torchroute.py).  python tests/radius_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import radius_cases as rc
from torchroute import N, bits, soup_scene as scene


def to_host(res):
    """(offsets, dist, prim, u, v) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(bits(x)[:m].view(t) for x, t in zip(res[1:], (np.float32, np.uint32, np.float32, np.float32)))


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    pts = rc.point_records(rt, tris, n=N)
    want = rt.radius_search_bvh4(tris, ctx.read_bvh4(), pts)
    total = int(want[0][-1])
    assert total > N
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(pts).cuda()                # (n, 4) records, zero-copy
        sized = ctx.radius_search(rec)                    # capacity=None: one read of offsets[-1]
        roomy = ctx.radius_search(rec, capacity=total + 100, simple=True)
        split = ctx.radius_search(rec[:, :3].contiguous(), r_max=rec[:, 3].contiguous(), capacity=total)     # (n, 3) points + radii
        counts = ctx.radius_count(rec)
        assert all(x.is_cuda for x in sized) and sized[0].dtype == torch.int64 and sized[2].dtype == torch.uint32 and counts.dtype == torch.uint32
        assert len(sized[1]) == total and len(roomy[1]) == total + 100
        got = [to_host(sized), to_host(roomy), to_host(split)]
        cnt = bits(counts)
    for g in got:
        rc.assert_same_lists(g, want, ordered=True)
    assert np.array_equal(cnt, np.diff(want[0].astype(np.int64)).astype(np.uint32))
    rc.assert_same_lists(ctx.radius_search(pts), want, ordered=True)      # and the numpy route


def truncation_on_the_device_route(rt, ctx):
    """pt_radius_search itself, per kernel, into guarded device tensors (torchroute.truncation_on_the_device_route)."""
    tris = scene(rt, ctx)
    pts_h = rc.point_records(rt, tris, n=N)
    _, want, _ = tr.truncation_on_the_device_route(
        rt, ctx, pts_h, (0, rt.PT_RADIUS_SIMPLE_KERNEL, rt.PT_RADIUS_BRUTE_FORCE),
        lambda tree: rc.words(rt.radius_search_bvh4(tris, tree, pts_h, brute_force=tree is None)), ctx.radius_search_device, rc.GUARD)[-1]
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.radius_search(torch.from_numpy(pts_h).cuda(), capacity=len(want) - 1, brute_force=True)
    assert len(res[2]) == len(want) - 1 and np.array_equal(bits(res[2]), want[:-1, 1])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    tris = scene(rt, ctx)
    pts = torch.from_numpy(rc.point_records(rt, tris, n=N)).cuda()
    cap = 16 * N

    def sequence():
        return list(ctx.radius_search(pts, capacity=cap)) + [ctx.radius_count(pts)]
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    assert 0 < int(want[0][-1]) <= cap
    res = tr.returns_before_the_stream(sequence)
    m = int(want[0][-1])
    assert torch.equal(res[0], want[0]) and torch.equal(res[5].view(torch.int32), want[5].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32)[:m], b.view(torch.int32)[:m]) for a, b in zip(res[1:5], want[1:5]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    pts = rc.point_records(rt, tris, n=N)
    want = rt.radius_search_bvh4(tris, ctx.read_bvh4(), pts)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.radius_search(torch.from_numpy(pts).cuda(), capacity=int(want[0][-1])))
    rc.assert_same_lists(to_host(res), want, ordered=True)
    rc.assert_same_lists(ctx.radius_search(pts), rt.radius_search_bvh4(other, ctx.read_bvh4(), pts), ordered=True)


def errors(rt, ctx):
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); pts[:, 3] = 10.0
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((64,), dtype=torch.int32, device="cuda")
    pp, op, ep, cp = pts.data_ptr(), off.data_ptr(), ent.data_ptr(), cnt.data_ptr()
    search = (ctx.radius_search_device, [pp, 1, op, ep, 16, 0], [
        (0, 0), (2, 0), (3, 0),                           # null (NULL entries only with capacity 0)
        (0, pp + 4), (2, op + 4), (3, ep + 8),            # points and entries: 16-byte aligned, offsets: 8-byte aligned
        (5, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    count = (ctx.radius_count_device, [pp, 1, cp, 0], [(0, 0), (2, 0), (0, pp + 4), (2, cp + 2), (3, 8), (1, 1 << 32)])      # counts: 4-byte aligned
    one = np.zeros((1, 4), np.float32)
    tr.refusals(rt, ctx, [search, count], lambda: scene(rt, ctx), host=[lambda: ctx.radius_search(one), lambda: ctx.radius_count(one)],
                cpu=[lambda: ctx.radius_search(torch.zeros((4, 4))), lambda: ctx.radius_count(torch.zeros((4, 4)))])
    off.fill_(7); ent.fill_(7); cnt.fill_(7)
    torch.cuda.synchronize()
    ctx.radius_search_device(pp, 0, op, ep, 16)                                           # n = 0: offsets[0] = 0, nothing else
    ctx.radius_count_device(pp, 0, cp)
    ctx.radius_search_device(pp, 63, op + 8, 0, 0)                                        # offsets only (64 words from off[1] on), at an 8-byte aligned address
    ctx.synchronize()
    assert int(off[0]) == 0 and int(ent.min()) == 7 and int(ent.max()) == 7 and int(cnt.min()) == 7
    assert int(off[1]) == 0 and int(off[2]) == 3000                                        # the whole soup lies within 10 of the origin
    dist, prim = ctx.radius_search(np.float32([[0, 0, 0, 10]]))[1:3]                       # the context is still usable
    assert len(prim) == 3000 and np.all(np.isfinite(dist))


if __name__ == "__main__":
    tr.main(globals())
