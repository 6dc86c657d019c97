"""The torch-route cases of tests/test_gpu_closest_points.py, run in a child process each: torch is imported BEFORE the package there, so
that libmi355pt binds to torch's copy of the HIP runtime (as tests/rayquery_torch_cases.py does).  python tests/closest_torch_cases.py NAME"""
import os
import sys

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import closest_cases as cc  # noqa: E402
from scenes import TETRA, random_soup  # noqa: E402


def to_numpy(res):
    return [x.cpu().view(torch.int32).numpy() for x in res]


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
    bvh4 = gpu_ctx.read_bvh4()
    pts = cc.query_points(tris, 20000, 43)
    want = rt.closest_points_bvh4(tris, bvh4, pts)
    gpu_ctx.set_batch(8)
    for f in range(3):                                   # queued by pt_set_batch, not launched yet
        gpu_ctx.render(gpu_ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    res = gpu_ctx.closest_points(torch.from_numpy(pts).cuda())      # launches the three frames first, then the query
    other = random_soup(5000, 47)
    gpu_ctx.set_triangles(other); gpu_ctx.build_bvh()    # after the query: its results stay those of the first scene
    for a, b in zip(want, to_numpy(res)):
        assert cc.same_bits(a, b)
    after = gpu_ctx.closest_points(pts)                  # and the next query sees the second scene
    for a, b in zip(after, rt.closest_points_bvh4(other, gpu_ctx.read_bvh4(), pts)):
        assert cc.same_bits(a, b)


def errors(rt, gpu_ctx):
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    pp, op = pts.data_ptr(), out.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, op)) == 4                   # no scene
    assert code(lambda: gpu_ctx.closest_points(np.zeros((1, 3), np.float32))) == 4
    assert code(lambda: gpu_ctx.closest_points_device(pp + 4, 1, op)) == 1               # the pointers are checked before the scene
    gpu_ctx.set_triangles(TETRA)
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, op)) == 4                   # triangles without a tree
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, op, flags=rt.PT_CLOSEST_BRUTE_FORCE)) == 4
    gpu_ctx.build_bvh()
    assert code(lambda: gpu_ctx.closest_points_device(0, 1, op)) == 1                    # null
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, 0)) == 1
    assert code(lambda: gpu_ctx.closest_points_device(pp + 4, 1, op)) == 1               # not 16-byte aligned
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, op + 8)) == 1
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1, op, flags=8)) == 1          # unknown flag
    assert code(lambda: gpu_ctx.closest_points_device(pp, 1 << 32, op)) == 1             # n > UINT32_MAX
    out.fill_(7)
    torch.cuda.synchronize()
    gpu_ctx.closest_points_device(pp, 0, op)                                              # n = 0: OK, nothing launched
    gpu_ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    dist, prim, _, _ = gpu_ctx.closest_points(np.float32([[0, 0, 3]]))                    # the context is still usable
    assert prim[0] != cc.MISS and np.isfinite(dist[0])


if __name__ == "__main__":
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
