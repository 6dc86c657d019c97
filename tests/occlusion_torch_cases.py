"""The torch-route cases of tests/test_gpu_occlusion.py, one child process each (tests/torchroute.py).  python tests/occlusion_torch_cases.py NAME"""
import sys

import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

from routecheck import code
from scenes import TETRA
from test_gpu_occlusion import MISS, SCENE_SEED, composition, same_bits, scene, surface_surfels, traced_mask
from torchroute import bits


def to_numpy(res):
    return [bits(x) for x in res]


def torch_route_equals_the_host_route(rt, gpu_ctx):
    tris, _ = scene(rt, gpu_ctx, "soup120k")
    sf = surface_surfels(rt, tris, 20000, 53)
    host = [gpu_ctx.occlusion(sf, 16, seed=3, index_base=9, simple=simple) for simple in (False, True)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is; no synchronize
        sft = torch.from_numpy(sf).cuda()
        dev = [gpu_ctx.occlusion(sft, 16, seed=3, index_base=9, simple=simple) for simple in (False, True)]
        assert all(x.is_cuda for x in dev[0]) and dev[0][1].dtype == torch.uint32
        out = [to_numpy(d) for d in dev]
    for h, d in zip(host, out):
        for a, b in zip(h, d):
            assert same_bits(a, b)
    # a strided view is copied, not misread
    wide = torch.zeros((len(sf), 12), dtype=torch.float32, device="cuda"); wide[:, :8] = torch.from_numpy(sf).cuda()
    for a, b in zip(host[0], to_numpy(gpu_ctx.occlusion(wide[:, :8], 16, seed=3, index_base=9))):
        assert same_bits(a, b)


def device_rays_equal_the_host_twin(rt, gpu_ctx):
    """occlusion_rays_kernel writes the host twin's bits (which tests/test_occlusion_host.py pins to the oracle), for every ray; and the
    composition on the device -- occlusion_rays -> trace_rays(any_hit) -> a torch count -- equals pt_occlusion."""
    tris, _ = scene(rt, gpu_ctx, "soup1k")
    sf = surface_surfels(rt, tris, 5000, 57)
    sft = torch.from_numpy(sf).cuda()
    for samples, seed, base in ((1, 0, 0), (16, 7, 0xFFFFFF00), (100, 0xC0FFEE, 12345)):
        dev = gpu_ctx.occlusion_rays(sft, samples, seed=seed, index_base=base, bias=2e-4)
        assert dev.shape == (len(sf) * samples, 8)
        host = rt.occlusion_rays_host(sf, samples, seed=seed, index_base=base, bias=2e-4)
        got = dev.cpu().numpy()
        bad = np.flatnonzero((got.view(np.uint32) != host.view(np.uint32)).any(axis=1))
        assert len(bad) == 0, (samples, len(bad), bad[:5], got[bad[:2]], host[bad[:2]])
        _, prim, _, _ = gpu_ctx.trace_rays(dev, any_hit=True)
        miss = (prim.view(torch.int32) == -1).reshape(len(sf), samples).sum(dim=1)
        traced = torch.from_numpy(traced_mask(sf)).cuda()
        want = torch.where(traced, miss, torch.zeros_like(miss)).cpu().numpy().astype(np.uint32)
        _, unocc, smp = gpu_ctx.occlusion(sft, samples, seed=seed, index_base=base, bias=2e-4)
        assert np.array_equal(to_numpy([unocc])[0], want)
        assert np.array_equal(to_numpy([smp])[0], np.where(traced_mask(sf), samples, 0).astype(np.uint32))
    # hit_surfels on the device equals the host route
    from test_gpu_rayquery import random_rays
    O, D = random_rays(tris, 6000, 61)
    rays = rt.pack_rays(O, D)
    want = gpu_ctx.hit_surfels(rays, gpu_ctx.trace_rays(rays), 0.5)
    rt_ = torch.from_numpy(rays).cuda()
    got = gpu_ctx.hit_surfels(rt_, gpu_ctx.trace_rays(rt_), 0.5)
    assert got.is_cuda and same_bits(got.cpu().numpy(), want)


def no_host_synchronisation(rt, gpu_ctx):
    tris, _ = scene(rt, gpu_ctx, "soup1k")
    sf = torch.from_numpy(surface_surfels(rt, tris, 20000, 59)).cuda()

    def sequence():
        res = gpu_ctx.occlusion(sf, 16)
        rays = gpu_ctx.occlusion_rays(sf, 4)
        return res, gpu_ctx.hit_surfels(rays, gpu_ctx.trace_rays(rays), 1.0)
    res, surf = sequence()                                # warm-up
    want = to_numpy(res)
    del res, surf
    torch.cuda.synchronize()
    res, surf = tr.returns_before_the_stream(sequence)
    for a, b in zip(want, to_numpy(res)):
        assert same_bits(a, b)
    assert surf.shape == (len(sf) * 4, 8)


def ordering_with_batched_frames_and_scene_changes(rt, gpu_ctx):
    import orc as orc_mod
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    sf = surface_surfels(rt, tris, 5000, 43)
    want_u, want_s = composition(rt, gpu_ctx, sf, 16)
    (_, unocc, smp), _ = tr.queued_frames_then(rt, gpu_ctx, lambda: gpu_ctx.occlusion(torch.from_numpy(sf).cuda(), 16))
    assert np.array_equal(bits(unocc), want_u) and np.array_equal(bits(smp), want_s)
    tr.queued_frames_saw(orc_mod.load(), gpu_ctx, tris, bvh4)
    after, _ = composition(rt, gpu_ctx, sf, 16)          # and the new scene answers differently
    assert not np.array_equal(after, want_u)


def ao_pipeline(rt, gpu_ctx, w, h, samples, radius, seed):
    p = gpu_ctx.make_params(w, h)
    rays = gpu_ctx.camera_rays(p)
    hits = gpu_ctx.trace_rays(rays)
    sf = gpu_ctx.hit_surfels(rays, hits, radius)
    vis, unocc, smp = gpu_ctx.occlusion(sf, samples, seed=seed)
    return rays, hits, sf, vis, unocc, smp


def camera_pipeline_stays_on_the_device(rt, gpu_ctx):
    tris, _ = scene(rt, gpu_ctx, "dragon")
    w, h = 320, 180
    rays, hits, sf, vis, unocc, smp = ao_pipeline(rt, gpu_ctx, w, h, 16, float("inf"), 1)
    assert sf.is_cuda and vis.is_cuda
    prim = to_numpy([hits[1]])[0]
    hit = prim != MISS
    assert w * h // 20 < hit.sum() < w * h
    sfh = sf.cpu().numpy()
    assert np.array_equal(traced_mask(sfh), hit)
    u, s = to_numpy([unocc, smp])
    assert np.all(s[hit] == 16) and np.all(s[~hit] == 0) and np.all(vis.cpu().numpy()[~hit] == 0)
    want_u, want_s = composition(rt, gpu_ctx, sfh, 16, seed=1)
    assert np.array_equal(u, want_u) and np.array_equal(s, want_s)
    assert 0 < u[hit].sum() < 16 * hit.sum()


def errors(rt, gpu_ctx):
    sf = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); sf[:, 3] = float("inf"); sf[:, 6] = 1.0
    out = torch.zeros((64, 4), dtype=torch.int32, device="cuda"); rays = torch.zeros((64 * 4, 8), dtype=torch.float32, device="cuda")
    hits = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    sp, op, rp, hp = sf.data_ptr(), out.data_ptr(), rays.data_ptr(), hits.data_ptr()

    def params(samples=4, bias=1e-4, flags=0):
        p = rt.PtOcclusionParams(); p.samples, p.bias, p.flags = samples, bias, flags
        return p

    dev = gpu_ctx.occlusion_device
    occlusion = (dev, [sp, 1, params(), op], [
        (0, 0), (3, 0), (0, sp + 4), (3, op + 8),         # null, not 16-byte aligned
        (2, params(flags=4)), (2, params(samples=0)), (2, params(samples=65537)), (2, params(bias=-1.0)), (2, params(bias=float("nan")))])
    many = (dev, [sp, 1, params(samples=1), op], [(1, 1 << 32)])                              # n > UINT32_MAX
    product = (dev, [sp, 1, params(samples=65536), op], [(1, 65536)])                         # n * samples = 2^32
    assert code(rt, lambda: gpu_ctx.hit_surfels_device(rp, hp, 1, 1.0, sp)) == 4                # no scene
    gpu_ctx.occlusion_rays_device(sp, 64, params(), rp)                                       # needs no scene
    gpu_ctx.synchronize()
    assert same_bits(rays.cpu().numpy(), rt.occlusion_rays_host(sf.cpu().numpy(), 4))

    def tetra():
        gpu_ctx.set_triangles(TETRA); gpu_ctx.build_bvh()
    tr.refusals(rt, gpu_ctx, [occlusion, many, product], tetra, host=[lambda: gpu_ctx.occlusion(np.zeros((1, 8), np.float32), 4)],
                cpu=[lambda: gpu_ctx.occlusion(torch.zeros((4, 8)), 4)])
    assert code(rt, lambda: gpu_ctx.occlusion_rays_device(sp, 1, params(), 0)) == 1
    assert code(rt, lambda: gpu_ctx.occlusion_rays_device(sp, 1, params(), rp + 4)) == 1
    assert code(rt, lambda: gpu_ctx.hit_surfels_device(rp, hp, 1, 1.0, 0)) == 1
    assert code(rt, lambda: gpu_ctx.hit_surfels_device(rp, hp + 4, 1, 1.0, sp)) == 1
    assert code(rt, lambda: gpu_ctx.hit_surfels_device(rp, hp, 1 << 32, 1.0, sp)) == 1
    out.fill_(7)
    torch.cuda.synchronize()
    gpu_ctx.occlusion_device(sp, 0, params(), op)                                             # n = 0: OK, nothing launched
    gpu_ctx.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7
    gpu_ctx.occlusion_device(sp, 64, params(), op)                                            # the context is still usable
    gpu_ctx.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    assert np.all(o[:, 2] == 4) and np.all(o[:, 3] == 0) and np.all(o[:, 1] <= 4)


def ao_frame(rt, gpu_ctx):
    """What `main.js --tris 20000 --ao S --ao-radius R` computes, as width * height float32 visibilities: argv = W H S R OUT."""
    w, h, samples, radius, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]), sys.argv[6]
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000, SCENE_SEED)
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh()
    vis = ao_pipeline(rt, gpu_ctx, w, h, samples, radius, 1)[3]
    vis.cpu().numpy().astype(np.float32).tofile(out)


if __name__ == "__main__":
    tr.main(globals())
