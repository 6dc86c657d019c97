"""The torch-route cases of tests/test_gpu_sweep.py, one child process each (tests/torchroute.py).  python tests/sweep_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import sweep_cases as sc
from routecheck import assert_guarded, same_bits
from torchroute import N, bits, soup_scene as scene

GUARD = 0x5A5A5A5A


def to_host(res):
    return tuple(bits(x) for x in res)


def same(got, want):
    for a, b in zip(got, want):
        assert same_bits(a, b)


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
    for flags, tree in ((0, ctx.read_bvh4()), (rt.PT_SWEEP_SIMPLE_KERNEL, ctx.read_bvh4()), (rt.PT_SWEEP_BRUTE_FORCE, None)):
        want = np.stack([np.ascontiguousarray(w).view(np.uint32) for w in rt.sweep_spheres_bvh4(tris, tree, S, brute_force=tree is None)], axis=1)
        for n in (1, 64, N):
            out = tr.guarded(n + 8, GUARD)
            ctx.sweep_spheres_device(rec.data_ptr(), n, out.data_ptr(), flags)
            ctx.synchronize()
            assert_guarded(bits(out), want[:n], GUARD, (flags, n))


def no_host_synchronisation_then_a_scene_change(rt, ctx):
    """The call returns while earlier work of the stream is still running, and a scene change after it does not change its results."""
    tris = scene(rt, ctx)
    S = sc.sweep_set(rt, tris, N, 5)
    want = rt.sweep_spheres_bvh4(tris, ctx.read_bvh4(), S)
    rec = torch.from_numpy(S).cuda()
    ctx.sweep_spheres(rec)                                # warm-up
    torch.cuda.synchronize()
    res = tr.returns_before_the_stream(lambda: ctx.sweep_spheres(rec))
    other = tr.second_scene(ctx)                          # after the query: its results stay those of the first scene
    torch.cuda.synchronize()
    same(to_host(res), want)
    same(ctx.sweep_spheres(S), rt.sweep_spheres_bvh4(other, ctx.read_bvh4(), S))      # the next query sees the second


def errors(rt, ctx):
    rec = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); rec[:, 2] = 3.0; rec[:, 3] = float("inf"); rec[:, 6] = -1.0; rec[:, 7] = 0.1
    out = torch.full((64, 4), 7, dtype=torch.int32, device="cuda")
    pp, op = rec.data_ptr(), out.data_ptr()
    sweep = (ctx.sweep_spheres_device, [pp, 1, op, 0], [(0, 0), (2, 0), (0, pp + 4), (2, op + 8), (3, 8), (1, 1 << 32)])      # null, not 16-byte aligned, unknown flag, n > UINT32_MAX
    tr.refusals(rt, ctx, [sweep], lambda: scene(rt, ctx), host=[lambda: ctx.sweep_spheres(np.zeros((1, 8), np.float32))], cpu=[lambda: ctx.sweep_spheres(torch.zeros((4, 8)))])
    torch.cuda.synchronize()
    ctx.sweep_spheres_device(pp, 0, op)                                                   # n = 0: nothing is launched
    ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    t, prim, _, _ = ctx.sweep_spheres(rec)                                                # the context is still usable
    assert bool((prim.cpu().view(torch.int32) != -1).all()) and bool(torch.isfinite(t).all())


if __name__ == "__main__":
    tr.main(globals())
