"""The torch-route cases of tests/test_gpu_rayquery.py, run in a child process each: torch is imported BEFORE the package there, so that
libmi355pt binds to torch's copy of the HIP runtime (one process drives the GPU through one copy; bench.py imports torch first for the
same reason).  python tests/rayquery_torch_cases.py NAME"""
import os
import sys

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import orc as orc_mod  # noqa: E402
from scenes import TETRA, random_soup  # noqa: E402
from test_gpu_rayquery import MISS, oracle_batch, random_rays, same_bits, scene  # noqa: E402


def camera_rays_equal_a_mode_1_render_on_c2(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "dragon")
    w, h = 1920, 1080
    p = gpu_ctx.make_params(w, h)
    rays = gpu_ctx.camera_rays(p)
    t, prim, _, _ = gpu_ctx.trace_rays(rays, stats=True)
    st = gpu_ctx.stats()
    prim = prim.cpu().view(torch.int32).numpy().view(np.uint32); t = t.cpu().numpy()
    _, ids, ost = orc.render(orc.make_params(w, h, tris.size // 9, mode=orc_mod.MODE_SINGLE), tris, bvh4, want_tri_ids=True)
    assert np.array_equal(prim.reshape(h, w), ids)
    assert (prim != MISS).sum() > w * h // 20
    assert st["rays_closest"] == w * h and st["rays_shadow"] == 0
    for k in ("nodes_examined", "tris_tested", "stack_drops", "max_stack"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    t2, prim2, _, _ = gpu_ctx.trace_rays(rays)            # the persistent kernel
    assert same_bits(prim2.cpu().view(torch.int32).numpy(), prim) and same_bits(t2.cpu().numpy(), t)
    r = rays.cpu().numpy()                                 # origin = the camera, t_max = +inf, reserved = 0; the host route agrees
    assert np.all(r[:, 0:3] == np.float32([0, 0, 2.5])) and np.all(np.isposinf(r[:, 3])) and np.all(r[:, 7] == 0)
    _, prim3, _, _ = gpu_ctx.trace_rays(r)
    assert np.array_equal(prim3, prim)


def ordering_with_batched_frames_and_scene_changes(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup1k")
    O, D = random_rays(tris, 20000, 43)
    hit, ot, oprim = oracle_batch(orc, tris, bvh4, O, D)
    gpu_ctx.set_batch(8)
    for f in range(3):                                   # queued by pt_set_batch, not launched yet
        gpu_ctx.render(gpu_ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    rays = torch.from_numpy(rt.pack_rays(O, D)).cuda()
    t, prim, _, _ = gpu_ctx.trace_rays(rays)             # launches the three frames first, then the query
    other = random_soup(5000, 47)
    gpu_ctx.set_triangles(other); gpu_ctx.build_bvh()    # after the query: its results stay those of the first scene
    prim = prim.cpu().view(torch.int32).numpy().view(np.uint32); t = t.cpu().numpy()
    assert np.array_equal(prim != MISS, hit) and np.array_equal(prim[hit], oprim[hit]) and same_bits(t[hit], ot[hit])
    img = gpu_ctx.read_radiance(64, 48)                  # the queued frames saw the first scene
    ref, _, _ = orc.render(orc.make_params(64, 48, tris.size // 9, mode=orc_mod.MODE_SINGLE), tris, bvh4)
    assert same_bits(img, ref)


def torch_route_equals_the_host_route(rt, orc, gpu_ctx):
    tris, bvh4 = scene(rt, gpu_ctx, "soup120k")
    O, D = random_rays(tris, 50000, 53)
    host, host_any = gpu_ctx.trace_rays(O, D), gpu_ctx.trace_rays(O, D, any_hit=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is; no synchronize
        Ot, Dt = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
        dev = gpu_ctx.trace_rays(Ot, Dt)
        dev_any = gpu_ctx.trace_rays(Ot, Dt, any_hit=True, t_max=torch.full((len(O),), float("inf"), device="cuda"))
        out = [x.cpu().view(torch.int32).numpy() for x in dev + dev_any]
    for a, b in zip(host + host_any, out):
        assert same_bits(a, b)


def errors(rt, orc, gpu_ctx):
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); hits = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    rp, hp = rays.data_ptr(), hits.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1, hp)) == 4                     # no scene
    assert code(lambda: gpu_ctx.trace_rays(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))) == 4
    gpu_ctx.set_triangles(TETRA)
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1, hp)) == 4                     # triangles without a tree
    gpu_ctx.build_bvh()
    assert code(lambda: gpu_ctx.trace_rays_device(0, 1, hp)) == 1                      # null
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1, 0)) == 1
    assert code(lambda: gpu_ctx.trace_rays_device(rp + 4, 1, hp)) == 1                 # not 16-byte aligned
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1, hp + 8)) == 1
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1, hp, flags=8)) == 1            # unknown flag
    assert code(lambda: gpu_ctx.trace_rays_device(rp, 1 << 32, hp)) == 1               # n > UINT32_MAX
    assert code(lambda: gpu_ctx.camera_rays_device(gpu_ctx.make_params(8, 8), 0)) == 1
    assert code(lambda: gpu_ctx.camera_rays_device(gpu_ctx.make_params(8, 8), rp + 4)) == 1
    hits.fill_(7)
    torch.cuda.synchronize()
    gpu_ctx.trace_rays_device(rp, 0, hp)                                                # n = 0: OK, nothing launched
    gpu_ctx.synchronize()
    assert int(hits.min()) == 7 and int(hits.max()) == 7
    _, prim, _, _ = gpu_ctx.trace_rays(np.float32([[0, 0, 3]]), np.float32([[0, 0, -1]]))   # the context is still usable
    assert prim[0] != MISS


if __name__ == "__main__":
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, orc_mod.load(), ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
