"""The torch-route cases of tests/test_gpu_knn.py, run in a child process each: torch is imported BEFORE the package there, so that
libmi355pt binds to torch's copy of the HIP runtime (as tests/radius_torch_cases.py does).  python tests/knn_torch_cases.py NAME"""
import os
import sys
import time

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import knn_cases as kc  # noqa: E402
import radius_cases as rc  # noqa: E402
from scenes import random_soup  # noqa: E402

N = 4097
KS = (1, 4, 5, 16, 17, 64)


def scene(rt, ctx):
    tris = random_soup(3000, 5)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def points(rt, tris, n=N):
    pts = rc.point_records(rt, tris, n=n)
    pts[0::2, 3] = np.inf
    return pts


def to_host(res):
    """(dist, prim, u, v) of (n, k) torch tensors -> the numpy form of the host route"""
    return tuple(x.contiguous().cpu().view(torch.int32).numpy().view(t) for x, t in zip(res, (np.float32, np.uint32, np.float32, np.float32)))


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
    guard = int(np.uint32(rc.GUARD).astype(np.int32))
    b4 = ctx.read_bvh4()
    for flags, tree, n in ((0, b4, N), (rt.PT_NEAREST_SIMPLE_KERNEL, b4, N), (rt.PT_NEAREST_BRUTE_FORCE, None, 513)):
        for k in KS:
            want = kc.words(rt.nearest_k_bvh4(tris, tree, pts_h[:n], k, brute_force=tree is None)).reshape(n * k, 4)
            buf = torch.full((n * k + 8, 4), guard, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.nearest_k_device(pts.data_ptr(), n, k, buf.data_ptr(), flags)
            ctx.synchronize()
            got = buf.cpu().numpy().view(np.uint32)
            kc.assert_guard(got, n, k)
            assert np.array_equal(got[:n * k], want), (flags, k, np.flatnonzero((got[:n * k] != want).any(1))[:8])


def no_host_synchronisation(rt, ctx):
    """The call returns while earlier work of the stream is still running: behind a long spin kernel on torch's stream it comes back, and an
    event recorded after it has not completed yet."""
    tris = scene(rt, ctx)
    pts = torch.from_numpy(points(rt, tris)).cuda()

    def sequence():
        return [x for k in (4, 16, 64) for x in ctx.nearest_k(pts, k)]
    want = sequence()                                     # warm-up: first-touch allocations may wait, a steady-state call does not
    torch.cuda.synchronize()
    t0 = time.perf_counter(); torch.cuda._sleep(5_000_000); torch.cuda.synchronize(); probe = time.perf_counter() - t0
    cycles = int(min(max(5_000_000 * 0.3 / probe, 5_000_000), 2_000_000_000))      # about 0.3 s, whatever the counter's rate
    t0 = time.perf_counter(); torch.cuda._sleep(cycles); torch.cuda.synchronize(); spin = time.perf_counter() - t0
    assert spin > 0.05, spin                              # the spin is long enough to tell
    torch.cuda._sleep(cycles)
    t0 = time.perf_counter()
    res = sequence()
    took = time.perf_counter() - t0
    done = torch.cuda.Event(); done.record()
    pending = not done.query()
    torch.cuda.synchronize()
    assert pending and took < spin / 2, (pending, took, spin)
    assert all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(res, want))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    bvh4 = ctx.read_bvh4()
    pts = points(rt, tris)
    want = rt.nearest_k_bvh4(tris, bvh4, pts, 16)
    ctx.set_batch(8)
    for f in range(3):                                    # queued by pt_set_batch, not launched yet
        ctx.render(ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    res = ctx.nearest_k(torch.from_numpy(pts).cuda(), 16)      # launches the three frames first, then the query
    other = random_soup(5000, 47)
    ctx.set_triangles(other); ctx.build_bvh()             # after the query: its results stay those of the first scene
    kc.assert_same_rows(to_host(res), want)
    kc.assert_same_rows(ctx.nearest_k(pts, 16), rt.nearest_k_bvh4(other, ctx.read_bvh4(), pts, 16))      # the next query sees the second


def errors(rt, ctx):
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); pts[:, 3] = 10.0
    out = torch.full((64 * 64 + 8, 4), 7, dtype=torch.int32, device="cuda")
    pp, op = pts.data_ptr(), out.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: ctx.nearest_k_device(pp, 1, 3, op)) == 4                          # no scene
    assert code(lambda: ctx.nearest_k_device(pp + 4, 1, 3, op)) == 1                      # the pointers are checked before the scene
    scene(rt, ctx)
    assert code(lambda: ctx.nearest_k_device(0, 1, 3, op)) == 1                           # null
    assert code(lambda: ctx.nearest_k_device(pp, 1, 3, 0)) == 1
    assert code(lambda: ctx.nearest_k_device(pp + 4, 1, 3, op)) == 1                      # 16-byte aligned
    assert code(lambda: ctx.nearest_k_device(pp, 1, 3, op + 8)) == 1
    assert code(lambda: ctx.nearest_k_device(pp, 1, 0, op)) == 1                          # k
    assert code(lambda: ctx.nearest_k_device(pp, 1, 65, op)) == 1
    assert code(lambda: ctx.nearest_k_device(pp, 1, 3, op, flags=8)) == 1                 # unknown flag
    assert code(lambda: ctx.nearest_k_device(pp, 1 << 32, 3, op)) == 1                    # n > UINT32_MAX
    assert code(lambda: ctx.nearest_k(pts, 0)) == 1 and code(lambda: ctx.nearest_k(pts, 65)) == 1
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
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
