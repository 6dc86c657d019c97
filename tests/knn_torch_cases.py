"""The torch-route cases of tests/test_gpu_knn.py, one child process each (tests/torchroute.py).  python tests/knn_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import knn_cases as kc
import radius_cases as rc
from routecheck import assert_guarded, code
from torchroute import N, bits, soup_scene as scene

KS = (1, 4, 5, 16, 17, 64)


def points(rt, tris, n=N):
    pts = rc.point_records(rt, tris, n=n)
    pts[0::2, 3] = np.inf
    return pts


def to_host(res):
    """(dist, prim, u, v) of (n, k) torch tensors -> the numpy form of the host route"""
    return tuple(bits(x).view(t) for x, t in zip(res, (np.float32, np.uint32, np.float32, np.float32)))


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    pts = points(rt, tris)
    b4 = ctx.read_bvh4()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(pts).cuda()                # (n, 4) records, zero-copy
        got = {}
        for k in KS:
            res = ctx.nearest_k(rec, k)
            assert all(x.is_cuda and tuple(x.shape) == (N, k) for x in res) and res[1].dtype == torch.uint32 and res[0].dtype == torch.float32
            got[k] = to_host(res)
        simple = to_host(ctx.nearest_k(rec, 5, simple=True))
        split = to_host(ctx.nearest_k(rec[:, :3].contiguous(), 5, r_max=rec[:, 3].contiguous()))      # (n, 3) points + radii
        brute = to_host(ctx.nearest_k(rec[:256], 17, brute_force=True))
    for k in KS:
        kc.assert_same_rows(got[k], rt.nearest_k_bvh4(tris, b4, pts, k))
    want = rt.nearest_k_bvh4(tris, b4, pts, 5)
    kc.assert_same_rows(simple, want); kc.assert_same_rows(split, want)
    kc.assert_same_rows(brute, rt.nearest_k_bvh4(tris, None, pts[:256], 17, brute_force=True))
    kc.assert_same_rows(ctx.nearest_k(pts, 5), want)      # and the numpy route


def guard_on_the_device_route(rt, ctx):
    """pt_nearest_k itself, per kernel and k: the rows go into a device tensor of n * k + 8 records filled with a guard pattern, so a store
    behind n * k lands where it is seen, and a record that is not written keeps the pattern."""
    tris = scene(rt, ctx)
    pts_h = points(rt, tris)
    pts_h[1::8, 3] = 0.0; pts_h[5::16, 0] = np.nan        # rows of points that are not walked are written too
    pts = torch.from_numpy(pts_h).cuda()
    b4 = ctx.read_bvh4()
    for flags, tree, n in ((0, b4, N), (rt.PT_NEAREST_SIMPLE_KERNEL, b4, N), (rt.PT_NEAREST_BRUTE_FORCE, None, 513)):
        for k in KS:
            want = kc.words(rt.nearest_k_bvh4(tris, tree, pts_h[:n], k, brute_force=tree is None)).reshape(n * k, 4)
            buf = tr.guarded(n * k + 8, rc.GUARD)
            ctx.nearest_k_device(pts.data_ptr(), n, k, buf.data_ptr(), flags)
            ctx.synchronize()
            got = bits(buf)
            kc.assert_guard(got, n, k)
            assert_guarded(got, want, rc.GUARD, (flags, k))


def no_host_synchronisation(rt, ctx):
    tris = scene(rt, ctx)
    pts = torch.from_numpy(points(rt, tris)).cuda()

    def sequence():
        return [x for k in (4, 16, 64) for x in ctx.nearest_k(pts, k)]
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    res = tr.returns_before_the_stream(sequence)
    assert all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(res, want))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    pts = points(rt, tris)
    want = rt.nearest_k_bvh4(tris, ctx.read_bvh4(), pts, 16)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.nearest_k(torch.from_numpy(pts).cuda(), 16))
    kc.assert_same_rows(to_host(res), want)
    kc.assert_same_rows(ctx.nearest_k(pts, 16), rt.nearest_k_bvh4(other, ctx.read_bvh4(), pts, 16))


def errors(rt, ctx):
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); pts[:, 3] = 10.0
    out = torch.full((64 * 64 + 8, 4), 7, dtype=torch.int32, device="cuda")
    pp, op = pts.data_ptr(), out.data_ptr()
    nearest = (ctx.nearest_k_device, [pp, 1, 3, op, 0], [
        (0, 0), (3, 0), (0, pp + 4), (3, op + 8),         # null, not 16-byte aligned
        (2, 0), (2, 65),                                  # k
        (4, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    tr.refusals(rt, ctx, [nearest], lambda: scene(rt, ctx), host=[lambda: ctx.nearest_k(np.zeros((1, 4), np.float32), 3)], cpu=[lambda: ctx.nearest_k(torch.zeros((4, 4)), 3)])
    assert code(rt, lambda: ctx.nearest_k(pts, 0)) == 1 and code(rt, lambda: ctx.nearest_k(pts, 65)) == 1
    torch.cuda.synchronize()
    ctx.nearest_k_device(pp, 0, 3, op)                                                    # n = 0: nothing is written
    ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    ctx.nearest_k_device(pp, 64, 64, op)                                                  # the largest k
    ctx.synchronize()
    rows = out.cpu().numpy().view(np.uint32)
    assert np.all(rows[64 * 64:] == 7) and np.all(rows[:64 * 64, 1] < 3000)                # the whole soup lies within 10 of the origin
    dist, prim = ctx.nearest_k(np.float32([[0, 0, 0, 10]]), 8)[:2]                         # the context is still usable
    assert prim.shape == (1, 8) and np.all(np.isfinite(dist)) and np.all(np.diff(dist[0]) >= 0)


if __name__ == "__main__":
    tr.main(globals())
