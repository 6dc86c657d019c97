"""The torch-route cases of tests/test_gpu_cut.py, one child process each (tests/torchroute.py).  python tests/cut_torchroute_cases.py NAME"""
import torchroute as tr      # first: it imports torch before the package

import numpy as np
import torch

import cut_cases as ctc
from torchroute import N, bits, soup_scene as scene


def planes(rt, tris):
    """N planes with windows twice the size of cut_cases': more than N entries over the 3000-triangle soup, as the shared cases ask"""
    rec = ctc.plane_records(rt, tris, n=N, beside=0)
    c = (rec[:, 4:7] + rec[:, 8:11]) * np.float32(0.5)
    h = (rec[:, 8:11] - rec[:, 4:7]) * np.float32(1.0)
    rec[:, 4:7], rec[:, 8:11] = c - h, c + h
    return rec


def to_host(res):
    """(offsets, prim, code, t0, t1) of torch tensors -> the numpy form of the host route, cut at the total (t0 and t1 as float32)"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64), bits(res[1])[:m], bits(res[2])[:m], bits(res[3])[:m].view(np.float32), bits(res[4])[:m].view(np.float32))


def torch_route_equals_the_host_route(rt, ctx):
    tris = scene(rt, ctx)
    rec_h = planes(rt, tris)
    want = rt.cut_search_bvh4(tris, ctx.read_bvh4(), rec_h)
    total = int(want[0][-1])
    assert total > N
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                            # ordered with torch's current stream, whichever it is
        rec = torch.from_numpy(rec_h).cuda()              # (n, 12) records, zero-copy
        sized = ctx.cut_search(rec)                       # capacity=None: one read of offsets[-1]
        roomy = ctx.cut_search(rec, capacity=total + 100, simple=True)
        split = ctx.cut_search(rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 8:11], capacity=total)       # normal, d, lo, hi
        counts = ctx.cut_count(rec)
        assert all(x.is_cuda for x in sized) and sized[0].dtype == torch.int64 and sized[1].dtype == torch.uint32 and sized[2].dtype == torch.uint32
        assert sized[3].dtype == torch.float32 and sized[4].dtype == torch.float32
        assert counts.dtype == torch.uint32 and len(sized[1]) == total and len(roomy[1]) == total + 100
        got = [to_host(sized), to_host(roomy), to_host(split)]
        cnt = bits(counts)
    for g in got:
        ctc.assert_same_lists(g, want, ordered=True)
    assert np.array_equal(cnt, np.diff(want[0].astype(np.int64)).astype(np.uint32))
    ctc.assert_same_lists(ctx.cut_search(rec_h), want, ordered=True)      # and the numpy route
    # one normal and one d for every window, the windows on the device
    one = ctx.cut_search(rec[0, 0:3], float(rec_h[0, 3]), rec[:64, 4:7], rec[:64, 8:11], capacity=4096)
    tiled = rec_h[:64].copy(); tiled[:, 0:4] = rec_h[0, 0:4]
    ctc.assert_same_lists(to_host(one), rt.cut_search_bvh4(tris, ctx.read_bvh4(), tiled), ordered=True)


def truncation_on_the_device_route(rt, ctx):
    """pt_cut_search itself, per kernel, into guarded device tensors (torchroute.truncation_on_the_device_route)."""
    tris = scene(rt, ctx)
    rec_h = planes(rt, tris)

    def twin(tree):
        full = rt.cut_search_bvh4(tris, tree, rec_h, brute_force=tree is None)
        return ctc.words(full)[0], ctc.records_of(full)
    _, want, _ = tr.truncation_on_the_device_route(rt, ctx, rec_h, (0, rt.PT_CUT_SIMPLE_KERNEL, rt.PT_CUT_BRUTE_FORCE), twin, ctx.cut_search_device, ctc.GUARD)[-1]
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.cut_search(torch.from_numpy(rec_h).cuda(), capacity=len(want) - 1, brute_force=True)
    assert len(res[1]) == len(want) - 1 and np.array_equal(bits(res[1]), want[:-1, 0]) and np.array_equal(bits(res[4]), want[:-1, 3])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    tris = scene(rt, ctx)
    rec = torch.from_numpy(planes(rt, tris)).cuda()
    cap = 32 * N

    def sequence():
        return list(ctx.cut_search(rec, capacity=cap)) + [ctx.cut_count(rec)]
    want = sequence()                                     # warm-up
    torch.cuda.synchronize()
    assert 0 < int(want[0][-1]) <= cap
    res = tr.returns_before_the_stream(sequence)
    m = int(want[0][-1])
    assert torch.equal(res[0], want[0]) and torch.equal(res[5].view(torch.int32), want[5].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32)[:m], b.view(torch.int32)[:m]) for a, b in zip(res[1:5], want[1:5]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    rec = planes(rt, tris)
    want = rt.cut_search_bvh4(tris, ctx.read_bvh4(), rec)
    res, other = tr.queued_frames_then(rt, ctx, lambda: ctx.cut_search(torch.from_numpy(rec).cuda(), capacity=int(want[0][-1])))
    ctc.assert_same_lists(to_host(res), want, ordered=True)
    ctc.assert_same_lists(ctx.cut_search(rec), rt.cut_search_bvh4(other, ctx.read_bvh4(), rec), ordered=True)


def errors(rt, ctx):
    span = rt.pack_cuts([0.3, 0.5, 0.9], 0.0, [-10, -10, -10], [10, 10, 10])             # cuts through the whole soup
    rec = torch.from_numpy(np.tile(span, (64, 1))).cuda()
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((64,), dtype=torch.int32, device="cuda")
    pp, op, ep, cp = rec.data_ptr(), off.data_ptr(), ent.data_ptr(), cnt.data_ptr()
    search = (ctx.cut_search_device, [pp, 1, op, ep, 16, 0], [
        (0, 0), (2, 0), (3, 0),                           # null (NULL entries only with capacity 0)
        (0, pp + 4), (2, op + 4), (3, ep + 8),            # planes and entries: 16-byte aligned, offsets: 8-byte aligned
        (5, 8), (1, 1 << 32)])                            # unknown flag, n > UINT32_MAX
    count = (ctx.cut_count_device, [pp, 1, cp, 0], [(0, 0), (2, 0), (0, pp + 4), (2, cp + 2), (3, 8), (1, 1 << 32)])      # counts: 4-byte aligned
    one = np.zeros((1, 12), np.float32)
    tris = []
    tr.refusals(rt, ctx, [search, count], lambda: tris.append(scene(rt, ctx)), host=[lambda: ctx.cut_search(one), lambda: ctx.cut_count(one)],
                cpu=[lambda: ctx.cut_search(torch.zeros((4, 12))), lambda: ctx.cut_count(torch.zeros((4, 12)))])
    tr.raises_value_error(lambda: ctx.cut_search(rec[:, :5]))                              # neither (n, 12) records nor a normal and d
    cut = int(rt.cut_search_bvh4(tris[0], None, span, brute_force=True)[0][-1])
    assert cut > 16
    off.fill_(7); ent.fill_(7); cnt.fill_(7)
    torch.cuda.synchronize()
    ctx.cut_search_device(pp, 0, op, ep, 16)                                              # n = 0: offsets[0] = 0, nothing else
    ctx.cut_count_device(pp, 0, cp)
    ctx.cut_search_device(pp, 63, op + 8, 0, 0)                                           # offsets only (64 words from off[1] on), at an 8-byte aligned address
    ctx.synchronize()
    assert int(off[0]) == 0 and int(ent.min()) == 7 and int(ent.max()) == 7 and int(cnt.min()) == 7
    assert int(off[1]) == 0 and int(off[2]) == cut
    _, prim, code, t0, t1 = ctx.cut_search(span)                                           # the context is still usable
    assert len(prim) == cut and np.all(np.isin(code & 7, (3, 5, 6)))


if __name__ == "__main__":
    tr.main(globals())
