"""The torch-route cases of tests/test_gpu_crossings.py, one child process each (tests/torchroute.py).  python tests/crossings_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import crossing_cases as cc
from routecheck import same_bits
from scenes import TETRA
from torchroute import bits

N_RAYS, N_POINTS = 4096, 2048


def to_numpy(res):
    return [bits(x) for x in res]


def scene(rt, ctx, name="torus"):
    tris = cc.geometry(rt, name)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    rays = cc.ray_set(rt, tris, N_RAYS, 31)
    pts = rt.pack_points(cc.cube_points(N_POINTS, 37, half=1.0), 0.1)
    host_c = [ctx.count_hits(rays, simple=s) for s in (False, True)] + [ctx.count_hits(rays, brute_force=True)]
    host_in = [ctx.contains(pts, samples=3, seed=4, simple=s) for s in (False, True)]
    host_sd = ctx.signed_distance(pts, samples=3, seed=4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is; no synchronize
        rt_, pt_ = torch.from_numpy(rays).cuda(), torch.from_numpy(pts).cuda()
        dev_c = [ctx.count_hits(rt_, simple=s_) for s_ in (False, True)] + [ctx.count_hits(rt_, brute_force=True)]
        dev_in = [ctx.contains(pt_, samples=3, seed=4, simple=s_) for s_ in (False, True)]
        dev_sd = ctx.signed_distance(pt_, samples=3, seed=4)
        assert dev_c[0].is_cuda and dev_c[0].dtype == torch.uint32 and dev_in[0][0].dtype == torch.uint32 and dev_sd[0].dtype == torch.float32
        got_c, got_in, got_sd = to_numpy(dev_c), [to_numpy(d) for d in dev_in], to_numpy(dev_sd)
    assert all(np.array_equal(a, b) for a, b in zip(host_c, got_c))
    assert all(np.array_equal(a, b) for h, d in zip(host_in, got_in) for a, b in zip(h, d))
    assert all(same_bits(a, b) for a, b in zip(host_sd, got_sd))
    # (n, 3) points and separate origins / directions; a strided view is copied, not misread
    assert np.array_equal(to_numpy([ctx.count_hits(rt_[:, 0:3], rt_[:, 4:7], rt_[:, 3])])[0], host_c[0])
    wide = torch.zeros((len(pts), 6), dtype=torch.float32, device="cuda"); wide[:, :4] = pt_
    assert all(np.array_equal(a, b) for a, b in zip(host_in[0], to_numpy(ctx.contains(wide[:, :4], samples=3, seed=4))))
    assert all(np.array_equal(a, b) for a, b in zip(host_in[0], to_numpy(ctx.contains(wide[:, :3], samples=3, seed=4))))
    assert all(same_bits(a, b) for a, b in zip(host_sd, to_numpy(ctx.signed_distance(wide[:, :3], 0.1, samples=3, seed=4))))


def device_composition(rt, ctx):
    """pt_contains equals occlusion_rays -> count_hits -> a torch parity count, all on the device; and the signed distance is
    closest_points with the sign of contains."""
    scene(rt, ctx)
    pts = cc.cube_points(N_POINTS, 43, half=1.0)
    pts[5, 1] = np.nan
    sft = torch.from_numpy(cc.surfels_of(pts)).cuda()
    sft[5, 3] = 0.0                                        # the surfel of a point that is not traced
    pt_ = torch.from_numpy(pts).cuda()
    for samples, seed, base in ((1, 0, 0), (3, 7, 0xFFFFFF00), (7, 0xC0FFEE, 12345)):
        rays = ctx.occlusion_rays(sft, samples, seed=seed, index_base=base, bias=0.0)
        counts = ctx.count_hits(rays)
        odd = (counts.view(torch.int32) & 1).reshape(len(pts), samples).sum(dim=1)
        for simple in (False, True):
            inside, got_odd, smp = ctx.contains(pt_, samples=samples, seed=seed, index_base=base, simple=simple)
            assert torch.equal(got_odd.view(torch.int32), odd.to(torch.int32))
            assert torch.equal(inside.view(torch.int32), (2 * odd > samples).to(torch.int32))
            s = bits(smp)
            assert s[5] == 0 and np.all(np.delete(s, 5) == samples)
        dist, prim, u, v = ctx.closest_points(pt_)
        sd, sprim, su, sv = ctx.signed_distance(pt_, samples=samples, seed=seed, index_base=base)
        assert torch.equal(sd.abs().view(torch.int32), dist.view(torch.int32)) and torch.equal(sprim.view(torch.int32), prim.view(torch.int32))
        assert torch.equal(su.view(torch.int32), u.view(torch.int32)) and torch.equal(sv.view(torch.int32), v.view(torch.int32))
        assert torch.equal(torch.signbit(sd), inside.view(torch.int32) != 0)
    assert 0 < int((odd > 0).sum()) < len(pts)


def no_host_synchronisation(rt, ctx):
    tris = scene(rt, ctx)
    rays = torch.from_numpy(cc.ray_set(rt, tris, N_RAYS, 47)).cuda()
    pts = torch.from_numpy(cc.cube_points(N_POINTS, 53, half=1.0)).cuda()

    def sequence():
        return [ctx.count_hits(rays)] + list(ctx.contains(pts, samples=3)) + list(ctx.signed_distance(pts, samples=3))
    want = to_numpy(sequence())                            # warm-up
    torch.cuda.synchronize()
    res = tr.returns_before_the_stream(sequence)
    assert all(same_bits(a, b) for a, b in zip(want, to_numpy(res)))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    import orc as orc_mod
    tris = scene(rt, ctx)
    bvh4 = ctx.read_bvh4()
    rays = cc.ray_set(rt, tris, N_RAYS, 59)
    pts = cc.cube_points(N_POINTS, 61, half=1.0)
    want = [ctx.count_hits(rays)] + list(ctx.contains(pts, samples=3)) + list(ctx.signed_distance(pts, samples=3))
    rt_, pt_ = torch.from_numpy(rays).cuda(), torch.from_numpy(pts).cuda()
    got, _ = tr.queued_frames_then(rt, ctx, lambda: [ctx.count_hits(rt_)] + list(ctx.contains(pt_, samples=3)) + list(ctx.signed_distance(pt_, samples=3)))
    assert all(same_bits(a, b) for a, b in zip(want, to_numpy(got)))
    tr.queued_frames_saw(orc_mod.load(), ctx, tris, bvh4)
    assert not np.array_equal(ctx.count_hits(rays), want[0])      # and the new scene answers differently


def errors(rt, ctx):
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); rays[:, 3] = float("inf"); rays[:, 2] = 3.0; rays[:, 6] = -1.0; rays[:, 0] = 0.2
    pts = torch.zeros((64, 4), dtype=torch.float32, device="cuda"); pts[:, 3] = float("inf")
    counts = torch.zeros((64,), dtype=torch.int32, device="cuda"); out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    rp, pp, cp, op = rays.data_ptr(), pts.data_ptr(), counts.data_ptr(), out.data_ptr()

    def params(samples=3, flags=0):
        return rt.PtContainParams(samples, 0, 0, flags)
    count = (ctx.count_hits_device, [rp, 1, cp, 0], [
        (0, 0), (2, 0), (0, rp + 4), (2, cp + 2),         # null, rays not 16-byte aligned, counts not 4-byte aligned
        (3, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    bad = [(0, 0), (3, 0), (0, pp + 4), (3, op + 8), (2, params(flags=4)), (2, params(samples=0)), (2, params(samples=2)), (2, params(samples=256)),
           (1, (1 << 32) // 3 + 1)]                       # n * samples > 2^32 - 1
    inside, signed = ((fn, [pp, 1, params(), op], bad) for fn in (ctx.contains_device, ctx.signed_distance_device))

    def tetra():
        ctx.set_triangles(TETRA); ctx.build_bvh()
    one = np.zeros((1, 3), np.float32)
    tr.refusals(rt, ctx, [count, inside, signed], tetra,
                host=[lambda: ctx.count_hits(rt.pack_rays(one, one + 1)), lambda: ctx.contains(one), lambda: ctx.signed_distance(one)],
                cpu=[lambda: ctx.count_hits(torch.zeros((4, 8))), lambda: ctx.contains(torch.zeros((4, 4))), lambda: ctx.signed_distance(torch.zeros((4, 4)))])
    counts.fill_(7); out.fill_(7)
    torch.cuda.synchronize()
    ctx.count_hits_device(rp, 0, cp); ctx.contains_device(pp, 0, params(), op); ctx.signed_distance_device(pp, 0, params(), op)      # n = 0: OK, nothing launched
    ctx.synchronize()
    assert int(counts.min()) == 7 and int(out.min()) == 7 and int(out.max()) == 7
    ctx.count_hits_device(rp, 64, cp + 4 * 0)                                              # the context is still usable
    ctx.contains_device(pp, 64, params(), op)
    ctx.synchronize()
    assert counts.cpu().tolist() == [2] * 64
    assert out.cpu().numpy().view(np.uint32).tolist() == [[1, 3, 3, 0]] * 64
    ctx.count_hits_device(rp + 32, 63, cp + 4)                                             # counts need 4-byte alignment only
    ctx.synchronize()
    assert counts.cpu().tolist() == [2] * 64


if __name__ == "__main__":
    tr.main(globals())
