"""The torch-route cases of tests/test_gpu_closest_points.py, one child process each (tests/torchroute.py).
python tests/closest_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import closest_cases as cc
from scenes import TETRA, random_soup
from torchroute import bits


def to_numpy(res):
    return [bits(x) for x in res]


def torch_route_equals_the_host_route(rt, gpu_ctx):
    tris = random_soup(120000, 5, size=0.02)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = cc.query_points(tris, 50000, 53)
    host = gpu_ctx.closest_points(pts)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is; no synchronize
        pt = torch.from_numpy(pts).cuda()
        dev = gpu_ctx.closest_points(pt)                  # (n, 3) points
        rec = gpu_ctx.closest_points(torch.from_numpy(rt.pack_points(pts)).cuda(), simple=True)      # (n, 4) records, zero-copy
        half = gpu_ctx.closest_points(pt, r_max=torch.full((len(pts),), 0.05, device="cuda"))
        assert all(x.is_cuda for x in dev) and dev[1].dtype == torch.uint32
        out = to_numpy(dev) + to_numpy(rec) + to_numpy(half)
    for a, b in zip(host + host, out[:8]):
        assert cc.same_bits(a, b)
    want = gpu_ctx.closest_points(pts, r_max=0.05)
    for a, b in zip(want, out[8:]):
        assert cc.same_bits(a, b)
    assert 0 < (want[1] != cc.MISS).sum() < len(pts)


def ordering_with_batched_frames_and_scene_changes(rt, gpu_ctx):
    tris = random_soup(1000, 3)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    pts = cc.query_points(tris, 20000, 43)
    want = rt.closest_points_bvh4(tris, gpu_ctx.read_bvh4(), pts)
    res, other = tr.queued_frames_then(rt, gpu_ctx, lambda: gpu_ctx.closest_points(torch.from_numpy(pts).cuda()))
    for a, b in zip(want, to_numpy(res)):
        assert cc.same_bits(a, b)
    for a, b in zip(gpu_ctx.closest_points(pts), rt.closest_points_bvh4(other, gpu_ctx.read_bvh4(), pts)):      # the next query sees the second scene
        assert cc.same_bits(a, b)


def errors(rt, gpu_ctx):
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    pp, op = pts.data_ptr(), out.data_ptr()
    closest = (gpu_ctx.closest_points_device, [pp, 1, op, 0], [(0, 0), (2, 0), (0, pp + 4), (2, op + 8), (3, 8), (1, 1 << 32)])      # null, not 16-byte aligned, unknown flag, n > UINT32_MAX
    brute = (gpu_ctx.closest_points_device, [pp, 1, op, rt.PT_CLOSEST_BRUTE_FORCE], [])      # brute force walks no tree, and needs the scene all the same

    def tetra():
        gpu_ctx.set_triangles(TETRA); gpu_ctx.build_bvh()
    tr.refusals(rt, gpu_ctx, [closest, brute], tetra, host=[lambda: gpu_ctx.closest_points(np.zeros((1, 3), np.float32))],
                cpu=[lambda: gpu_ctx.closest_points(torch.zeros((4, 4)))])
    out.fill_(7)
    torch.cuda.synchronize()
    gpu_ctx.closest_points_device(pp, 0, op)                                              # n = 0: OK, nothing launched
    gpu_ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    dist, prim, _, _ = gpu_ctx.closest_points(np.float32([[0, 0, 3]]))                    # the context is still usable
    assert prim[0] != cc.MISS and np.isfinite(dist[0])


if __name__ == "__main__":
    tr.main(globals())
