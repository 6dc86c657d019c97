"""The torch-route cases of tests/test_gpu_rayquery.py, one child process each (tests/torchroute.py).  python tests/rayquery_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import orc as orc_mod
from routecheck import code
from scenes import TETRA
from test_gpu_rayquery import MISS, oracle_batch, random_rays, same_bits, scene
from torchroute import bits


def camera_rays_equal_a_mode_1_render_on_c2(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "dragon")
    w, h = 1920, 1080
    p = gpu_ctx.make_params(w, h)
    rays = gpu_ctx.camera_rays(p)
    t, prim, _, _ = gpu_ctx.trace_rays(rays, stats=True)
    st = gpu_ctx.stats()
    prim = bits(prim); t = t.cpu().numpy()
    _, ids, ost = orc.render(orc.make_params(w, h, tris.size // 9, mode=orc_mod.MODE_SINGLE), tris, bvh4, want_tri_ids=True)
    assert np.array_equal(prim.reshape(h, w), ids)
    assert (prim != MISS).sum() > w * h // 20
    assert st["rays_closest"] == w * h and st["rays_shadow"] == 0
    for k in ("nodes_examined", "tris_tested", "stack_drops", "max_stack"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    t2, prim2, _, _ = gpu_ctx.trace_rays(rays)            # the persistent kernel
    assert same_bits(bits(prim2), prim) and same_bits(t2.cpu().numpy(), t)
    r = rays.cpu().numpy()                                 # origin = the camera, t_max = +inf, reserved = 0; the host route agrees
    assert np.all(r[:, 0:3] == np.float32([0, 0, 2.5])) and np.all(np.isposinf(r[:, 3])) and np.all(r[:, 7] == 0)
    _, prim3, _, _ = gpu_ctx.trace_rays(r)
    assert np.array_equal(prim3, prim)


def ordering_with_batched_frames_and_scene_changes(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    O, D = random_rays(tris, 20000, 43)
    hit, ot, oprim = oracle_batch(orc, tris, bvh4, O, D)
    (t, prim, _, _), _ = tr.queued_frames_then(rt, gpu_ctx, lambda: gpu_ctx.trace_rays(torch.from_numpy(rt.pack_rays(O, D)).cuda()))
    prim = bits(prim); t = t.cpu().numpy()
    assert np.array_equal(prim != MISS, hit) and np.array_equal(prim[hit], oprim[hit]) and same_bits(t[hit], ot[hit])
    tr.queued_frames_saw(orc, gpu_ctx, tris, bvh4)


def torch_route_equals_the_host_route(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup120k")
    O, D = random_rays(tris, 50000, 53)
    host, host_any = gpu_ctx.trace_rays(O, D), gpu_ctx.trace_rays(O, D, any_hit=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is; no synchronize
        Ot, Dt = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
        dev = gpu_ctx.trace_rays(Ot, Dt)
        dev_any = gpu_ctx.trace_rays(Ot, Dt, any_hit=True, t_max=torch.full((len(O),), float("inf"), device="cuda"))
        out = [bits(x) for x in dev + dev_any]
    for a, b in zip(host + host_any, out):
        assert same_bits(a, b)


def errors(rt, orc, gpu_ctx):
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); hits = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    rp, hp = rays.data_ptr(), hits.data_ptr()
    trace = (gpu_ctx.trace_rays_device, [rp, 1, hp, 0], [(0, 0), (2, 0), (0, rp + 4), (2, hp + 8), (3, 8), (1, 1 << 32)])      # null, not 16-byte aligned, unknown flag, n > UINT32_MAX

    def tetra():
        gpu_ctx.set_triangles(TETRA); gpu_ctx.build_bvh()
    tr.refusals(rt, gpu_ctx, [trace], tetra, host=[lambda: gpu_ctx.trace_rays(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))],
                cpu=[lambda: gpu_ctx.trace_rays(torch.zeros((4, 8)))])
    assert code(rt, lambda: gpu_ctx.camera_rays_device(gpu_ctx.make_params(8, 8), 0)) == 1
    assert code(rt, lambda: gpu_ctx.camera_rays_device(gpu_ctx.make_params(8, 8), rp + 4)) == 1
    hits.fill_(7)
    torch.cuda.synchronize()
    gpu_ctx.trace_rays_device(rp, 0, hp)                                                # n = 0: OK, nothing launched
    gpu_ctx.synchronize()
    assert int(hits.min()) == 7 and int(hits.max()) == 7
    _, prim, _, _ = gpu_ctx.trace_rays(np.float32([[0, 0, 3]]), np.float32([[0, 0, -1]]))   # the context is still usable
    assert prim[0] != MISS


if __name__ == "__main__":
    tr.main(globals(), with_orc=True)
