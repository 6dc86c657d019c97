"""The torch-route cases of tests/test_gpu_box.py, one child process each (tests/torchroute.py).  python tests/box_torch_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import box_cases as bc
from torchroute import N, bits, soup_scene as scene


def to_host(res):
    """(offsets, prim, verts_inside) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(bits(x)[:m] for x in res[1:])


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    boxes = bc.box_records(rt, tris, n=N)
    want = rt.box_search_bvh4(tris, ctx.read_bvh4(), boxes)
    total = int(want[0][-1])
    assert total > N
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(boxes).cuda()              # (n, 8) records, zero-copy
        sized = ctx.box_search(rec)                       # capacity=None: one read of offsets[-1]
        roomy = ctx.box_search(rec, capacity=total + 100, simple=True)
        split = ctx.box_search(rec[:, 0:3].contiguous(), rec[:, 4:7].contiguous(), capacity=total)     # (n, 3) corners
        counts = ctx.box_count(rec)
        assert all(x.is_cuda for x in sized) and sized[0].dtype == torch.int64 and sized[1].dtype == torch.uint32 and sized[2].dtype == torch.uint32
        assert counts.dtype == torch.uint32 and len(sized[1]) == total and len(roomy[1]) == total + 100
        got = [to_host(sized), to_host(roomy), to_host(split)]
        cnt = bits(counts)
    for g in got:
        bc.assert_same_lists(g, want, ordered=True)
    assert np.array_equal(cnt, np.diff(want[0].astype(np.int64)).astype(np.uint32))
    bc.assert_same_lists(ctx.box_search(boxes), want, ordered=True)      # and the numpy route


def truncation_on_the_device_route(rt, ctx):
    """pt_box_search itself, per kernel, into guarded device tensors (torchroute.truncation_on_the_device_route)."""
    tris = scene(rt, ctx)
    boxes_h = bc.box_records(rt, tris, n=N)

    def twin(tree):
        full = rt.box_search_bvh4(tris, tree, boxes_h, brute_force=tree is None)
        return bc.words(full)[0], bc.records_of(full)
    _, want, _ = tr.truncation_on_the_device_route(rt, ctx, boxes_h, (0, rt.PT_BOX_SIMPLE_KERNEL, rt.PT_BOX_BRUTE_FORCE), twin, ctx.box_search_device, bc.GUARD)[-1]
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.box_search(torch.from_numpy(boxes_h).cuda(), capacity=len(want) - 1, brute_force=True)
    assert len(res[1]) == len(want) - 1 and np.array_equal(bits(res[1]), want[:-1, 0])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    tris = scene(rt, ctx)
    boxes = torch.from_numpy(bc.box_records(rt, tris, n=N)).cuda()
    cap = 32 * N

    def sequence():
        return list(ctx.box_search(boxes, capacity=cap)) + [ctx.box_count(boxes)]
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    assert 0 < int(want[0][-1]) <= cap
    res = tr.returns_before_the_stream(sequence)
    m = int(want[0][-1])
    assert torch.equal(res[0], want[0]) and torch.equal(res[3].view(torch.int32), want[3].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32)[:m], b.view(torch.int32)[:m]) for a, b in zip(res[1:3], want[1:3]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    boxes = bc.box_records(rt, tris, n=N)
    want = rt.box_search_bvh4(tris, ctx.read_bvh4(), boxes)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.box_search(torch.from_numpy(boxes).cuda(), capacity=int(want[0][-1])))
    bc.assert_same_lists(to_host(res), want, ordered=True)
    bc.assert_same_lists(ctx.box_search(boxes), rt.box_search_bvh4(other, ctx.read_bvh4(), boxes), ordered=True)


def errors(rt, ctx):
    boxes = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); boxes[:, 0:3] = -10.0; boxes[:, 4:7] = 10.0
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((64,), dtype=torch.int32, device="cuda")
    pp, op, ep, cp = boxes.data_ptr(), off.data_ptr(), ent.data_ptr(), cnt.data_ptr()
    search = (ctx.box_search_device, [pp, 1, op, ep, 16, 0], [
        (0, 0), (2, 0), (3, 0),                           # null (NULL entries only with capacity 0)
        (0, pp + 4), (2, op + 4), (3, ep + 8),            # boxes and entries: 16-byte aligned, offsets: 8-byte aligned
        (5, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    count = (ctx.box_count_device, [pp, 1, cp, 0], [(0, 0), (2, 0), (0, pp + 4), (2, cp + 2), (3, 8), (1, 1 << 32)])      # counts: 4-byte aligned
    one = np.zeros((1, 8), np.float32)
    tr.refusals(rt, ctx, [search, count], lambda: scene(rt, ctx), host=[lambda: ctx.box_search(one), lambda: ctx.box_count(one)],
                cpu=[lambda: ctx.box_search(torch.zeros((4, 8))), lambda: ctx.box_count(torch.zeros((4, 8)))])
    tr.raises_value_error(lambda: ctx.box_search(boxes[:, :5]))                              # neither (n, 8) records nor lo and hi
    off.fill_(7); ent.fill_(7); cnt.fill_(7)
    torch.cuda.synchronize()
    ctx.box_search_device(pp, 0, op, ep, 16)                                              # n = 0: offsets[0] = 0, nothing else
    ctx.box_count_device(pp, 0, cp)
    ctx.box_search_device(pp, 63, op + 8, 0, 0)                                           # offsets only (64 words from off[1] on), at an 8-byte aligned address
    ctx.synchronize()
    assert int(off[0]) == 0 and int(ent.min()) == 7 and int(ent.max()) == 7 and int(cnt.min()) == 7
    assert int(off[1]) == 0 and int(off[2]) == 3000                                        # the whole soup lies in [-10, 10]^3
    _, prim, inside = ctx.box_search(np.float32([[-10, -10, -10]]), np.float32([[10, 10, 10]]))      # the context is still usable
    assert len(prim) == 3000 and np.all(inside == 7)


if __name__ == "__main__":
    tr.main(globals())
