"""The device-route contract of the batched queries, stated once for the child-process modules tests/*_torch_cases.py.  Each case runs in
a process of its own in which torch is imported BEFORE the package, so that libmi355pt binds to torch's copy of the HIP runtime (one
process drives the GPU through one copy; bench.py imports torch first for the same reason).  A child module imports this module first
and ends with

    if __name__ == "__main__":
        torchroute.main(globals())

What is here is what every query family asks of its torch route: the call returns while the stream is busy, it is ordered behind
queued frames and before a scene change, a list query never writes past its capacity, and bad arguments are refused before the scene
is looked at.  The torch-free parts (the guarded-buffer comparison, the error code of a call) are in tests/routecheck.py."""
import os
import sys
import time

import torch      # first

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import importlib  # noqa: E402

import numpy as np  # noqa: E402

from routecheck import assert_guarded, code, same_bits  # noqa: E402
from scenes import TETRA, random_soup  # noqa: E402

N = 4097          # 64 x 64 + 1 records: the last wavefront and the last chunk hold one item


def main(namespace, with_orc=False):
    """The __main__ of a child module: `python tests/X_torch_cases.py NAME [words the case reads from sys.argv]` runs namespace[NAME](rt, ctx),
    or NAME(rt, orc, ctx) with_orc, on a fresh context and prints "ok NAME"."""
    rt = importlib.import_module("raytracer-public_amd")
    assert rt._TORCH_FIRST
    head = (rt,)
    if with_orc:
        import orc as orc_mod
        head += (orc_mod.load(),)
    ctx = rt.Context(0)
    try:
        namespace[sys.argv[1]](*head, ctx)
    finally:
        ctx.close()
    print("ok", sys.argv[1])


def soup_scene(rt, ctx):
    tris = random_soup(3000, 5)
    ctx.set_triangles(tris); ctx.build_bvh()
    return tris


def bits(tensor):
    """a tensor of 4-byte words as a numpy uint32 array"""
    return tensor.contiguous().cpu().view(torch.int32).numpy().view(np.uint32)


def raises_value_error(call):
    """the binding itself refuses call(): a tensor that is not on the GPU, or of a shape that is no record"""
    try:
        call()
    except ValueError:
        return
    raise AssertionError("no error")


def returns_before_the_stream(call):
    """call() returns while earlier work of the stream is still running: behind a long spin kernel on torch's current stream it comes back,
    and an event recorded after it has not completed yet.  Returns call()'s result, with the stream still busy: whatever the caller does
    next is ordered behind the spin too.  The caller has made the same call once before (first-touch allocations may wait, a steady-state
    call does not) and synchronised."""
    t0 = time.perf_counter(); torch.cuda._sleep(5_000_000); torch.cuda.synchronize(); probe = time.perf_counter() - t0
    cycles = int(min(max(5_000_000 * 0.3 / probe, 5_000_000), 2_000_000_000))      # about 0.3 s, whatever the counter's rate
    t0 = time.perf_counter(); torch.cuda._sleep(cycles); torch.cuda.synchronize(); spin = time.perf_counter() - t0
    assert spin > 0.05, spin                              # the spin is long enough to tell
    torch.cuda._sleep(cycles)
    t0 = time.perf_counter()
    res = call()
    took = time.perf_counter() - t0
    done = torch.cuda.Event(); done.record()
    pending = not done.query()
    assert pending and took < spin / 2, (pending, took, spin)
    return res


def second_scene(ctx):
    """A scene change: what was queried before it keeps the first scene's results, the next query sees this one."""
    other = random_soup(5000, 47)
    ctx.set_triangles(other); ctx.build_bvh()
    return other


def queued_frames_then(rt, ctx, query):
    """Three frames queued by pt_set_batch and not launched yet, then query(), which launches them first, then a scene change: returns
    (what query() returned, the second scene's triangles).  The caller compares the first with the first scene's twin, and a query made
    afterwards with the second scene's."""
    ctx.set_batch(8)
    for f in range(3):
        ctx.render(ctx.make_params(64, 48, mode=rt.PT_MODE_REFERENCE, frame=f))
    res = query()
    return res, second_scene(ctx)


def queued_frames_saw(orc, ctx, tris, bvh4):
    """the frame that queued_frames_then left behind is the oracle's of the first scene"""
    import orc as orc_mod
    ref, _, _ = orc.render(orc.make_params(64, 48, tris.size // 9, mode=orc_mod.MODE_SINGLE), tris, bvh4)
    assert same_bits(ctx.read_radiance(64, 48), ref)


def guarded(rows, guard):
    """(rows, 4) int32 on the GPU, every word the guard pattern, and written before anything that follows"""
    buf = torch.full((rows, 4), int(np.uint32(guard).astype(np.int32)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return buf


def truncation_on_the_device_route(rt, ctx, records, kernels, twin, device, guard, more_capacities=lambda want_off: [], variants=((0, None),)):
    """A list query's raw entry point `device(records, n, offsets, entries, capacity, flags)`, per kernel, at the capacities 0 (NULL
    entries), total - 1, total and total + 7 (and the family's more_capacities(offsets)): the entries go into a device tensor of
    capacity + 8 records filled with a guard pattern, so a store at or beyond `capacity` lands where it is seen.  The offsets are complete
    whatever the capacity, the first min(total, capacity) records are the twin's, everything behind them is still the guard.

    records: the (N, w) numpy records; kernels: (tree flags, simple flags, brute-force flags); twin(tree): (offsets as int64, (total, 4)
    uint32 records) of the host twin over that tree, None being brute force; variants: (flag bits, expect(offsets, records, held)) pairs, expect
    None taking the twin's records as they are.  Returns (offsets, records, capacities) of each kernel."""
    rec = torch.from_numpy(records).cuda()
    seen = []
    for base, tree in zip(kernels, (ctx.read_bvh4(), ctx.read_bvh4(), None)):
        want_off, want = twin(tree)
        total = int(want_off[-1])
        assert total > N
        caps = [0, total - 1, total, total + 7] + list(more_capacities(want_off))
        for cap in caps:
            for bit, expect in variants:
                off = torch.full((N + 1,), -1, dtype=torch.int64, device="cuda")
                ent = guarded(cap + 8, guard)
                device(rec.data_ptr(), N, off.data_ptr(), ent.data_ptr() if cap else 0, cap, base | bit)
                ctx.synchronize()
                held = min(total, cap)
                assert_guarded(bits(ent), expect(want_off, want[:held], held) if expect else want[:held], guard, (base | bit, cap), (off.cpu().numpy(), want_off))
        seen.append((want_off, want, caps))
    return seen


def refusals(rt, ctx, queries, scene, host=(), cpu=()):
    """What a family's raw entry points refuse, on a context that has no scene yet.  queries: (call, good, bad) each, call(*good) being a
    valid call and bad a list of (index, value) overrides of one argument each, every one of them PT_ERR_INVALID_ARG (1): a null or
    misaligned pointer, an unknown flag, n = 1 << 32.  Before a scene the valid call is PT_ERR_NO_SCENE (4) and so is each of `host`, the
    host route's calls, while every override is 1 already: the arguments are checked before the scene.  Triangles without a tree are no
    scene either.  Then scene() installs the family's, every override is refused again, and each of `cpu`, which hands the torch route a tensor
    that is not on the GPU, raises ValueError."""
    def overrides():
        for call, good, bad in queries:
            for i, v in bad:
                args = list(good); args[i] = v
                assert code(rt, lambda: call(*args)) == 1, (call.__name__, i, v)

    def no_scene():
        for call, good, _ in queries:
            assert code(rt, lambda: call(*good)) == 4, call.__name__
    no_scene()
    for call in host:
        assert code(rt, call) == 4
    overrides()
    ctx.set_triangles(TETRA)
    no_scene()
    scene()
    overrides()
    for query in cpu:
        raises_value_error(query)
