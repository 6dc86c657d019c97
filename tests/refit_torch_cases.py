"""The torch-route cases of tests/test_gpu_refit.py, one child process each (tests/torchroute.py).  python tests/refit_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import orc as orc_mod
from refit_cases import wave
from routecheck import same_bits
from scenes import random_soup

SCENE_SEED = 20260109


def device_route_equals_the_host_route(rt, orc, gpu_ctx):
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 20000)
    moved = wave(tris, 0.1, 4)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(2)
    b4, b2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    gpu_ctx.update_triangles(moved)                          # the host route
    host4, host2 = gpu_ctx.read_bvh4(), gpu_ctx.read_bvh2()
    assert np.array_equal(host4, rt.refit_bvh4(moved, b4)) and np.array_equal(host2, rt.refit_bvh2(moved, b2))
    gpu_ctx.update_triangles(tris)
    p = gpu_ctx.make_params(160, 96, mode=rt.PT_MODE_PATH, spp=2, max_bounces=4, seed=3, stats=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                               # ordered with torch's current stream, whichever it is; no synchronize before the update
        t = torch.from_numpy(tris).cuda()
        x = t.view(-1, 3)[:, 0]
        # the wave of refit_cases.wave on the device: add, multiply, floor, abs round identically in torch float32
        u = (2 * x + 0.25) + 0.125 * 4
        t.view(-1, 3)[:, 1] += float(np.float32(0.1)) * (4 * (u - torch.floor(u) - 0.5).abs() - 1)
        gpu_ctx.update_triangles(t)
        gpu_ctx.render(p)                                    # plans with the refitted root box: waits for the 16-byte copy behind the refit
    gpu_ctx.synchronize()
    assert same_bits(t.cpu().numpy(), moved)
    t.fill_(float("nan"))                                    # after synchronize() the tensor is the caller's again: not read any more
    torch.cuda.synchronize()
    assert np.array_equal(gpu_ctx.read_bvh4(), host4) and np.array_equal(gpu_ctx.read_bvh2(), host2)
    ref, _, ost = orc.render(orc.make_params(160, 96, tris.size // 9, mode=orc_mod.MODE_PATH, spp=2, max_bounces=4, seed=3), moved, host4)
    assert same_bits(gpu_ctx.read_radiance(), ref)
    st = gpu_ctx.stats()
    for k in ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples"):
        assert st[k] == ost[k], k
    gpu_ctx.render(p)                                        # and a later frame still shows the update's geometry
    assert same_bits(gpu_ctx.read_radiance(), ref)
    # a tensor that is not float32 / contiguous is converted, one that is not on the GPU or not 9 floats per triangle is refused
    gpu_ctx.update_triangles(torch.from_numpy(tris.astype(np.float64)).cuda())
    gpu_ctx.synchronize()
    assert np.array_equal(gpu_ctx.read_bvh4(), b4)
    for bad in (torch.from_numpy(tris), torch.zeros(10, device="cuda")):
        tr.raises_value_error(lambda: gpu_ctx.update_triangles(bad))


def ordering_with_batched_frames(rt, orc, gpu_ctx):
    """set_batch(4): two frames, update, two frames -- each into a buffer of its own; each equals the oracle's frame for its own geometry."""
    tris = random_soup(3000, 11)
    n = tris.size // 9
    moved = wave(tris, 0.3, 2)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(2)
    old4 = gpu_ctx.read_bvh4()
    w, h = 128, 72
    bufs = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    gpu_ctx.set_batch(4)
    kw = dict(mode=rt.PT_MODE_PATH, spp=2, max_bounces=3, seed=8)
    for f in range(2):                                       # queued, not launched yet
        gpu_ctx.set_output_buffer(bufs[f].data_ptr(), w * h * 4)
        gpu_ctx.render(gpu_ctx.make_params(w, h, frame=f, **kw))
    gpu_ctx.update_triangles(torch.from_numpy(moved).cuda())  # launches the two frames first, then the refit
    for f in range(2, 4):
        gpu_ctx.set_output_buffer(bufs[f].data_ptr(), w * h * 4)
        gpu_ctx.render(gpu_ctx.make_params(w, h, frame=f, **kw))
    gpu_ctx.set_output_buffer(0, 0)                           # launches what is queued and waits
    new4 = gpu_ctx.read_bvh4()
    assert np.array_equal(new4, rt.refit_bvh4(moved, old4))
    for f in range(4):
        geo, tree = (tris, old4) if f < 2 else (moved, new4)
        ref, _, _ = orc.render(orc.make_params(w, h, n, mode=orc_mod.MODE_PATH, spp=2, max_bounces=3, seed=8, frame=f), geo, tree)
        assert same_bits(bufs[f].cpu().numpy(), ref), f
    a, _, _ = orc.render(orc.make_params(w, h, n, mode=orc_mod.MODE_PATH, spp=2, max_bounces=3, seed=8, frame=2), tris, old4)
    assert not same_bits(bufs[2].cpu().numpy(), a)           # the deformation is visible at all


def device_route_on_c2(rt, orc, gpu_ctx):
    """C2 at full size through the device route: words against the host twin."""
    tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED)
    moved = wave(tris, 0.1, 9)
    gpu_ctx.set_triangles(tris)
    gpu_ctx.build_bvh(0)
    b4 = gpu_ctx.read_bvh4()
    before = gpu_ctx.bvh_cost()
    gpu_ctx.update_triangles(torch.from_numpy(moved).cuda())
    got = gpu_ctx.read_bvh4()
    assert np.array_equal(got, rt.refit_bvh4(moved, b4))
    after, want = gpu_ctx.bvh_cost(), rt.bvh4_cost(got)
    assert abs(after - want) <= int(got[0]) * 2.0 ** -51 * want and after > before


if __name__ == "__main__":
    tr.main(globals(), with_orc=True)
