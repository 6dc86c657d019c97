import importlib, os, sys, time
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "/root/repo"))
rt = importlib.import_module("raytracer-public_amd")
# --moving-camera: a new camera position every frame, so every launch pays for a new tile cover -- the worst case of
# one render() per frame; without it the camera stands still and the cover is computed once
moving = "--moving-camera" in sys.argv[1:]
ctx = rt.Context(0); ctx.set_triangles(rt.procedural_scene(0, 871414)); ctx.build_bvh()
for name, mode, kw in (("reference", rt.PT_MODE_REFERENCE, {}), ("path", rt.PT_MODE_PATH, dict(spp=4, max_bounces=8))):
    p = ctx.make_params(1920, 1080, mode=mode, **kw)
    for _ in range(30): ctx.render(p)
    ctx.synchronize()
    n = 400
    t0 = time.perf_counter()
    for i in range(n):
        p.frame = i
        if moving: p.cam_pos[0] = 1e-4 * (i + 1)
        ctx.render(p)
    t1 = time.perf_counter(); ctx.synchronize(); t2 = time.perf_counter()
    print("%s%s: submit %.1f us per render() call, total %.3f ms per frame" % (name, " (moving camera)" if moving else "", (t1 - t0) / n * 1e6, (t2 - t0) / n * 1e3))
