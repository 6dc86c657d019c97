"""The torch-route cases of tests/test_gpu_sweep.py, run in a child process each: torch is imported BEFORE the package there, so that
libmi355pt binds to torch's copy of the HIP runtime (as tests/box_torch_cases.py does).  python tests/sweep_torch_cases.py NAME"""
import os
import sys
import time

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import sweep_cases as sc  # noqa: E402
from scenes import random_soup  # noqa: E402

N = 4097
GUARD = 0x5A5A5A5A


def scene(rt, ctx):
    tris = random_soup(3000, 5)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def to_host(res):
    return tuple(x.cpu().view(torch.int32).numpy().view(np.uint32) for x in res)


def same(got, want):
    for a, b in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    S = sc.sweep_set(rt, tris, N, 3)
    want = rt.sweep_spheres_bvh4(tris, ctx.read_bvh4(), S)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(S).cuda()                  # (n, 8) records, zero-copy
        whole = ctx.sweep_spheres(rec)
        simple = ctx.sweep_spheres(rec, simple=True)
        split = ctx.sweep_spheres(rec[:, 0:3].contiguous(), rec[:, 4:7].contiguous(), radius=rec[:, 7].contiguous(), t_max=rec[:, 3].contiguous())
        assert all(x.is_cuda for x in whole) and whole[0].dtype == torch.float32 and whole[1].dtype == torch.uint32
        got = [to_host(whole), to_host(simple), to_host(split)]
        wider = to_host(ctx.sweep_spheres(rec, radius=0.125, t_max=2.0))                  # an override on packed records: on a copy
        assert torch.equal(rec.cpu(), torch.from_numpy(S))                                # the caller's records are not written
    for g in got:
        same(g, want)
    same(wider, rt.sweep_spheres_bvh4(tris, ctx.read_bvh4(), S, radius=0.125, t_max=2.0))
    keep = S.copy()
    same(ctx.sweep_spheres(S, radius=0.125, t_max=2.0), wider)                            # the numpy route with the override: S keeps its bits
    assert np.array_equal(S.view(np.uint32), keep.view(np.uint32))
    same(ctx.sweep_spheres(S), want)                                                      # and the numpy route
    same(ctx.sweep_spheres(S[:, 0:3], S[:, 4:7], radius=S[:, 7], t_max=S[:, 3]), want)


def device_route_into_guarded_tensors(rt, ctx):
    """pt_sweep_spheres itself, per kernel: the hits go into a device tensor of n + 8 records filled with a guard pattern, so a store
    beyond the batch lands where it is seen."""
    tris = scene(rt, ctx)
    S = sc.sweep_set(rt, tris, N, 4)
    rec = torch.from_numpy(S).cuda()
    guard = int(np.uint32(GUARD).astype(np.int32))
    for flags, tree in ((0, ctx.read_bvh4()), (rt.PT_SWEEP_SIMPLE_KERNEL, ctx.read_bvh4()), (rt.PT_SWEEP_BRUTE_FORCE, None)):
        want = rt.sweep_spheres_bvh4(tris, tree, S, brute_force=tree is None)
        for n in (1, 64, N):
            out = torch.full((n + 8, 4), guard, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.sweep_spheres_device(rec.data_ptr(), n, out.data_ptr(), flags)
            ctx.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.all(got[n:] == GUARD), (flags, n)
            for k in range(4):
                assert np.array_equal(got[:n, k], np.ascontiguousarray(want[k][:n]).view(np.uint32)), (flags, n, k)


def no_host_synchronisation_then_a_scene_change(rt, ctx):
    """The call returns while earlier work of the stream is still running, and a scene change after it does not change its results."""
    tris = scene(rt, ctx)
    S = sc.sweep_set(rt, tris, N, 5)
    want = rt.sweep_spheres_bvh4(tris, ctx.read_bvh4(), S)
    rec = torch.from_numpy(S).cuda()
    ctx.sweep_spheres(rec)                                # warm-up: first-touch allocations may wait, a steady-state call does not
    torch.cuda.synchronize()
    t0 = time.perf_counter(); torch.cuda._sleep(5_000_000); torch.cuda.synchronize(); probe = time.perf_counter() - t0
    cycles = int(min(max(5_000_000 * 0.3 / probe, 5_000_000), 2_000_000_000))      # about 0.3 s, whatever the counter's rate
    t0 = time.perf_counter(); torch.cuda._sleep(cycles); torch.cuda.synchronize(); spin = time.perf_counter() - t0
    assert spin > 0.05, spin
    torch.cuda._sleep(cycles)
    t0 = time.perf_counter()
    res = ctx.sweep_spheres(rec)
    took = time.perf_counter() - t0
    done = torch.cuda.Event(); done.record()
    pending = not done.query()
    other = random_soup(5000, 47)
    ctx.set_triangles(other); ctx.build_bvh()             # after the query: its results stay those of the first scene
    torch.cuda.synchronize()
    assert pending and took < spin / 2, (pending, took, spin)
    same(to_host(res), want)
    same(ctx.sweep_spheres(S), rt.sweep_spheres_bvh4(other, ctx.read_bvh4(), S))      # the next query sees the second


def errors(rt, ctx):
    rec = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); rec[:, 2] = 3.0; rec[:, 3] = float("inf"); rec[:, 6] = -1.0; rec[:, 7] = 0.1
    out = torch.full((64, 4), 7, dtype=torch.int32, device="cuda")
    pp, op = rec.data_ptr(), out.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: ctx.sweep_spheres_device(pp, 1, op)) == 4                          # no scene
    assert code(lambda: ctx.sweep_spheres_device(pp + 4, 1, op)) == 1                      # the pointers are checked before the scene
    assert code(lambda: ctx.sweep_spheres(np.zeros((1, 8), np.float32))) == 4              # the host route
    scene(rt, ctx)
    assert code(lambda: ctx.sweep_spheres_device(0, 1, op)) == 1                           # null
    assert code(lambda: ctx.sweep_spheres_device(pp, 1, 0)) == 1
    assert code(lambda: ctx.sweep_spheres_device(pp + 4, 1, op)) == 1                      # 16-byte aligned
    assert code(lambda: ctx.sweep_spheres_device(pp, 1, op + 8)) == 1
    assert code(lambda: ctx.sweep_spheres_device(pp, 1, op, flags=8)) == 1                 # unknown flag
    assert code(lambda: ctx.sweep_spheres_device(pp, 1 << 32, op)) == 1                    # n > UINT32_MAX
    try:
        ctx.sweep_spheres(torch.zeros((4, 8)))                                            # a CPU tensor
        raise AssertionError("no error")
    except ValueError:
        pass
    torch.cuda.synchronize()
    ctx.sweep_spheres_device(pp, 0, op)                                                   # n = 0: nothing is launched
    ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    t, prim, _, _ = ctx.sweep_spheres(rec)                                                # the context is still usable
    assert bool((prim.cpu().view(torch.int32) != -1).all()) and bool(torch.isfinite(t).all())


if __name__ == "__main__":
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
