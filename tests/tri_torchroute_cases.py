"""The torch-route cases of tests/test_gpu_tri.py, one child process each (tests/torchroute.py).  python tests/tri_torchroute_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import tri_cases as tc
from torchroute import N, bits, soup_scene as scene


def callers(rt, tris):
    """N caller triangles twice the size of tri_cases': more than N entries over the 3000-triangle soup, as the shared cases ask"""
    return tc.caller_records(rt, tris, n=N, jitter=(2 * tc.J_LO, 2 * tc.J_HI))


def to_host(res):
    """(offsets, prim, edges) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(bits(x)[:m] for x in res[1:])


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    rec_h = callers(rt, tris)
    want = rt.tri_search_bvh4(tris, ctx.read_bvh4(), rec_h)
    total = int(want[0][-1])
    assert total > N
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(rec_h).cuda()              # (n, 12) records, zero-copy
        verts = rec.reshape(-1, 3, 4)[:, :, :3]
        sized = ctx.tri_search(rec)                       # capacity=None: one read of offsets[-1]
        roomy = ctx.tri_search(rec, capacity=total + 100, simple=True)
        split = ctx.tri_search(verts, capacity=total)     # (n, 3, 3) vertices
        flat = ctx.tri_search(verts.reshape(-1, 9), capacity=total)
        counts = ctx.tri_count(rec)
        pairs, edges = ctx.intersecting_pairs(rec)
        assert all(x.is_cuda for x in sized) and sized[0].dtype == torch.int64 and sized[1].dtype == torch.uint32 and sized[2].dtype == torch.uint32
        assert counts.dtype == torch.uint32 and len(sized[1]) == total and len(roomy[1]) == total + 100
        assert pairs.is_cuda and pairs.dtype == torch.int64 and tuple(pairs.shape) == (total, 2)
        got = [to_host(sized), to_host(roomy), to_host(split), to_host(flat)]
        cnt, pairs, edges = bits(counts), pairs.cpu().numpy(), bits(edges)
    for g in got:
        tc.assert_same_lists(g, want, ordered=True)
    assert np.array_equal(cnt, np.diff(want[0].astype(np.int64)).astype(np.uint32))
    assert np.array_equal(pairs[:, 0], tc.owner(want[0].astype(np.int64))) and np.array_equal(pairs[:, 1], want[1]) and np.array_equal(edges, want[2])
    tc.assert_same_lists(ctx.tri_search(rec_h), want, ordered=True)      # and the numpy route


def truncation_on_the_device_route(rt, ctx):
    """pt_tri_search itself, per kernel, into guarded device tensors (torchroute.truncation_on_the_device_route)."""
    tris = scene(rt, ctx)
    rec_h = callers(rt, tris)

    def twin(tree):
        full = rt.tri_search_bvh4(tris, tree, rec_h, brute_force=tree is None)
        return tc.words(full)[0], tc.records_of(full)
    _, want, _ = tr.truncation_on_the_device_route(rt, ctx, rec_h, (0, rt.PT_TRI_SIMPLE_KERNEL, rt.PT_TRI_BRUTE_FORCE), twin, ctx.tri_search_device, tc.GUARD)[-1]
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.tri_search(torch.from_numpy(rec_h).cuda(), capacity=len(want) - 1, brute_force=True)
    assert len(res[1]) == len(want) - 1 and np.array_equal(bits(res[1]), want[:-1, 0])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    tris = scene(rt, ctx)
    rec = torch.from_numpy(callers(rt, tris)).cuda()
    cap = 32 * N

    def sequence():
        return list(ctx.tri_search(rec, capacity=cap)) + [ctx.tri_count(rec)]
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    assert 0 < int(want[0][-1]) <= cap
    res = tr.returns_before_the_stream(sequence)
    m = int(want[0][-1])
    assert torch.equal(res[0], want[0]) and torch.equal(res[3].view(torch.int32), want[3].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32)[:m], b.view(torch.int32)[:m]) for a, b in zip(res[1:3], want[1:3]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    rec = callers(rt, tris)
    want = rt.tri_search_bvh4(tris, ctx.read_bvh4(), rec)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.tri_search(torch.from_numpy(rec).cuda(), capacity=int(want[0][-1])))
    tc.assert_same_lists(to_host(res), want, ordered=True)
    tc.assert_same_lists(ctx.tri_search(rec), rt.tri_search_bvh4(other, ctx.read_bvh4(), rec), ordered=True)


def errors(rt, ctx):
    span = np.float32([[-10, -10, -10, 0, 30, -10, 10, 0, -10, 30, 10, 0]])                # cuts through the whole soup
    rec = torch.from_numpy(np.tile(span, (64, 1))).cuda()
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((64,), dtype=torch.int32, device="cuda")
    pp, op, ep, cp = rec.data_ptr(), off.data_ptr(), ent.data_ptr(), cnt.data_ptr()
    search = (ctx.tri_search_device, [pp, 1, op, ep, 16, 0], [
        (0, 0), (2, 0), (3, 0),                           # null (NULL entries only with capacity 0)
        (0, pp + 4), (2, op + 4), (3, ep + 8),            # triangles and entries: 16-byte aligned, offsets: 8-byte aligned
        (5, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    count = (ctx.tri_count_device, [pp, 1, cp, 0], [(0, 0), (2, 0), (0, pp + 4), (2, cp + 2), (3, 8), (1, 1 << 32)])      # counts: 4-byte aligned
    one = np.zeros((1, 12), np.float32)
    tris = []
    tr.refusals(rt, ctx, [search, count], lambda: tris.append(scene(rt, ctx)), host=[lambda: ctx.tri_search(one), lambda: ctx.tri_count(one)],
                cpu=[lambda: ctx.tri_search(torch.zeros((4, 12))), lambda: ctx.tri_count(torch.zeros((4, 12)))])
    tr.raises_value_error(lambda: ctx.tri_search(rec[:, :5]))                              # neither (n, 12) records nor vertices
    cut = int(rt.tri_search_bvh4(tris[0], None, span, brute_force=True)[0][-1])
    assert cut > 16
    off.fill_(7); ent.fill_(7); cnt.fill_(7)
    torch.cuda.synchronize()
    ctx.tri_search_device(pp, 0, op, ep, 16)                                              # n = 0: offsets[0] = 0, nothing else
    ctx.tri_count_device(pp, 0, cp)
    ctx.tri_search_device(pp, 63, op + 8, 0, 0)                                           # offsets only (64 words from off[1] on), at an 8-byte aligned address
    ctx.synchronize()
    assert int(off[0]) == 0 and int(ent.min()) == 7 and int(ent.max()) == 7 and int(cnt.min()) == 7
    assert int(off[1]) == 0 and int(off[2]) == cut
    _, prim, edges = ctx.tri_search(span)                                                  # the context is still usable
    assert len(prim) == cut and np.all(edges != 0)


if __name__ == "__main__":
    tr.main(globals())
