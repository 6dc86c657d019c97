"""The torch-route cases of tests/test_gpu_box.py, run in a child process each: torch is imported BEFORE the package there, so that
libmi355pt binds to torch's copy of the HIP runtime (as tests/radius_torch_cases.py does).  python tests/box_torch_cases.py NAME"""
import os
import sys
import time

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

import box_cases as bc  # noqa: E402
from scenes import random_soup  # noqa: E402

N = 4097


def scene(rt, ctx):
    tris = random_soup(3000, 5)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def to_host(res):
    """(offsets, prim, verts_inside) of torch tensors -> the numpy form of the host route, cut at the total"""
    off = res[0].cpu().numpy()
    m = int(off[-1])
    return (off.astype(np.uint64),) + tuple(x.cpu().view(torch.int32).numpy()[:m].view(np.uint32) for x in res[1:])


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
        cnt = counts.cpu().view(torch.int32).numpy().view(np.uint32)
    for g in got:
        bc.assert_same_lists(g, want, ordered=True)
    assert np.array_equal(cnt, np.diff(want[0].astype(np.int64)).astype(np.uint32))
    bc.assert_same_lists(ctx.box_search(boxes), want, ordered=True)      # and the numpy route


def truncation_on_the_device_route(rt, ctx):
    """pt_box_search itself, per kernel, at the capacities 0 (NULL entries), total - 1, total and total + 7: the entries go into a device
    tensor of capacity + 8 records filled with a guard pattern, so a store at or beyond `capacity` lands where it is seen."""
    tris = scene(rt, ctx)
    boxes_h = bc.box_records(rt, tris, n=N)
    boxes = torch.from_numpy(boxes_h).cuda()
    guard = np.uint32(bc.GUARD).astype(np.int32)
    for flags, tree in ((0, ctx.read_bvh4()), (rt.PT_BOX_SIMPLE_KERNEL, ctx.read_bvh4()), (rt.PT_BOX_BRUTE_FORCE, None)):
        full = rt.box_search_bvh4(tris, tree, boxes_h, brute_force=tree is None)
        want_off, want = bc.words(full)[0], bc.records_of(full)
        total = int(want_off[-1])
        assert total > N
        for cap in (0, total - 1, total, total + 7):
            off = torch.full((N + 1,), -1, dtype=torch.int64, device="cuda")
            ent = torch.full((cap + 8, 4), int(guard), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.box_search_device(boxes.data_ptr(), N, off.data_ptr(), ent.data_ptr() if cap else 0, cap, flags)
            ctx.synchronize()
            got = ent.cpu().numpy().view(np.uint32)
            held = min(total, cap)
            assert np.array_equal(off.cpu().numpy(), want_off), (flags, cap)                  # complete whatever the capacity
            assert np.array_equal(got[:held], want[:held]), (flags, cap, np.flatnonzero((got[:held] != want[:held]).any(1))[:8])
            assert np.all(got[held:] == bc.GUARD), (flags, cap, np.flatnonzero((got[held:] != bc.GUARD).any(1))[:8] + held)
    # the torch route with a capacity below the total: the entry tensors hold `capacity` records, all of them written
    res = ctx.box_search(boxes, capacity=total - 1, brute_force=True)
    assert len(res[1]) == total - 1 and np.array_equal(res[1].cpu().view(torch.int32).numpy().view(np.uint32), want[:total - 1, 0])


def no_host_synchronisation_with_a_capacity(rt, ctx):
    """The call returns while earlier work of the stream is still running: behind a long spin kernel on torch's stream it comes back, and an
    event recorded after it has not completed yet."""
    tris = scene(rt, ctx)
    boxes = torch.from_numpy(bc.box_records(rt, tris, n=N)).cuda()
    cap = 32 * N

    def sequence():
        return list(ctx.box_search(boxes, capacity=cap)) + [ctx.box_count(boxes)]
    want = sequence()                                     # warm-up: first-touch allocations may wait, a steady-state call does not
    torch.cuda.synchronize()
    assert 0 < int(want[0][-1]) <= cap
    t0 = time.perf_counter(); torch.cuda._sleep(5_000_000); torch.cuda.synchronize(); probe = time.perf_counter() - t0
    cycles = int(min(max(5_000_000 * 0.3 / probe, 5_000_000), 2_000_000_000))      # about 0.3 s, whatever the counter's rate
    t0 = time.perf_counter(); torch.cuda._sleep(cycles); torch.cuda.synchronize(); spin = time.perf_counter() - t0
    assert spin > 0.05, spin                              # the spin is long enough to tell
    torch.cuda._sleep(cycles)
    t0 = time.perf_counter()
    res = sequence()
    took = time.perf_counter() - t0
    done = torch.cuda.Event(); done.record()
    pending = not done.query()
    torch.cuda.synchronize()
    assert pending and took < spin / 2, (pending, took, spin)
    m = int(want[0][-1])
    assert torch.equal(res[0], want[0]) and torch.equal(res[3].view(torch.int32), want[3].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32)[:m], b.view(torch.int32)[:m]) for a, b in zip(res[1:3], want[1:3]))


def ordering_with_batched_frames_and_scene_changes(rt, ctx):
    tris = scene(rt, ctx)
    bvh4 = ctx.read_bvh4()
    boxes = bc.box_records(rt, tris, n=N)
    want = rt.box_search_bvh4(tris, bvh4, boxes)
    ctx.set_batch(8)
    for f in range(3):                                    # queued by pt_set_batch, not launched yet
        ctx.render(ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    res = ctx.box_search(torch.from_numpy(boxes).cuda(), capacity=int(want[0][-1]))      # launches the three frames first, then the query
    other = random_soup(5000, 47)
    ctx.set_triangles(other); ctx.build_bvh()             # after the query: its results stay those of the first scene
    bc.assert_same_lists(to_host(res), want, ordered=True)
    bc.assert_same_lists(ctx.box_search(boxes), rt.box_search_bvh4(other, ctx.read_bvh4(), boxes), ordered=True)      # the next query sees the second


def errors(rt, ctx):
    boxes = torch.zeros((64, 8), dtype=torch.float32, device="cuda"); boxes[:, 0:3] = -10.0; boxes[:, 4:7] = 10.0
    off = torch.zeros((65,), dtype=torch.int64, device="cuda"); ent = torch.zeros((1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((64,), dtype=torch.int32, device="cuda")
    pp, op, ep, cp = boxes.data_ptr(), off.data_ptr(), ent.data_ptr(), cnt.data_ptr()

    def code(fn):
        try:
            fn()
        except rt.PtError as e:
            return e.code
        raise AssertionError("no error")
    assert code(lambda: ctx.box_search_device(pp, 1, op, ep, 16)) == 4                    # no scene
    assert code(lambda: ctx.box_count_device(pp, 1, cp)) == 4
    assert code(lambda: ctx.box_search_device(pp + 4, 1, op, ep, 16)) == 1                # the pointers are checked before the scene
    scene(rt, ctx)
    assert code(lambda: ctx.box_search_device(0, 1, op, ep, 16)) == 1                     # null
    assert code(lambda: ctx.box_search_device(pp, 1, 0, ep, 16)) == 1
    assert code(lambda: ctx.box_search_device(pp, 1, op, 0, 16)) == 1                     # NULL entries only with capacity 0
    assert code(lambda: ctx.box_search_device(pp + 4, 1, op, ep, 16)) == 1                # boxes: 16-byte aligned
    assert code(lambda: ctx.box_search_device(pp, 1, op + 4, ep, 16)) == 1                # offsets: 8-byte aligned
    assert code(lambda: ctx.box_search_device(pp, 1, op, ep + 8, 16)) == 1                # entries: 16-byte aligned
    assert code(lambda: ctx.box_count_device(pp, 1, cp + 2)) == 1                         # counts: 4-byte aligned
    assert code(lambda: ctx.box_count_device(pp, 1, 0)) == 1
    assert code(lambda: ctx.box_search_device(pp, 1, op, ep, 16, flags=8)) == 1           # unknown flag
    assert code(lambda: ctx.box_search_device(pp, 1 << 32, op, ep, 16)) == 1              # n > UINT32_MAX
    try:
        ctx.box_search(torch.zeros((4, 8)))                                               # a CPU tensor
        raise AssertionError("no error")
    except ValueError:
        pass
    try:
        ctx.box_search(boxes[:, :5])                                                      # neither (n, 8) records nor lo and hi
        raise AssertionError("no error")
    except ValueError:
        pass
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
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    ctx = rt.Context(0)
    try:
        globals()[sys.argv[1]](rt, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])
