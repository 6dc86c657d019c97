"""The megakernel's work queue against its restatement in exact integers (tests/queuemodel.py), over the plans the host really makes under
overridden knobs (pt_debug_launch_plan_tuned: pt_api.cpp::plan_launch with a PtTune filled from (name, value) pairs) -- no GPU.

For every plan that is not refused: every real batch is handed out exactly once under any order of claims and every padded item is
invalid; no cursor passes 2^32 - 1 (by the model's own count of atomic adds, not by the host's guard); the 32-bit range arithmetic of the
XCD-aware queue equals the exact one; the clamps hold.  The magic division is exact for every divisor a plan can produce.  And the
generated rows of the GPU knob lattice (tests/knob_lattice.py) cover every pair of levels of every two factors."""
import importlib
import itertools
import random
import re

import numpy as np
import pytest

import knob_lattice as kl
import queuemodel as qm

rt = importlib.import_module("raytracer-public_amd")

CUS = 256
C2_BATCHES = 97 * 92 * 4            # the traced batches of one C2 frame (tests/test_launch_plan.py)
K_MAX_SLOTS = 16                    # PtContext::kMaxSlots
REFUSALS = ("pt_render: batch too large (more than 2^32 items per launch)",
            "pt_render: launch too large for the 32-bit work-queue cursor (more than 2^32 - grid * chunk items; lower spp, the resolution or the batch)")
WAVES_PER_GROUP = int(re.search(r"workgroup (\d+)", rt.lib.pt_version().decode()).group(1)) // 64
FRAMES = (1, 2, 3, 5, 8, 9, 20, 32, 256)
TILE_COUNTS = (1, 2, 3, 8, 16)
EXTREMES = {"GRIDDIV": (0, 1, 2, 1024, 0xFFFFFFFE), "ROWS": (0, 1, 7, 4096, 4097, 0xFFFFFFFE), "CHUNK": (0, 1, 64, 65, 192, 1000, 4096, 1 << 20, 1 << 29, 1 << 30, 1 << 31, 0xFFFFFFC0, 0xFFFFFFFE),
            "XCD": (0, 1, 2, 0xFFFFFFFE), "SLOTS": (0, 1, 2, 15, 16, 17, 0xFFFFFFFE)}


def plan_or_refusal(frames, tile_count, batches, tune, cus=CUS, in_flight=0):
    try:
        return rt.debug_launch_plan_tuned(cus, frames, tile_count, in_flight, batches, frames, tune), None
    except rt.PtError as e:
        return None, str(e).split(": ", 1)[1]


def random_tune(rnd):
    tune = {}
    for name, ext in EXTREMES.items():
        r = rnd.random()
        if r < 0.35:
            continue
        if r < 0.7:
            tune[name] = rnd.choice(ext)
        else:
            tune[name] = {"GRIDDIV": rnd.randint(1, 8192), "ROWS": rnd.randint(1, 5000), "CHUNK": rnd.choice((rnd.randint(1, 700), rnd.randint(1, 1 << 16))),
                          "XCD": rnd.randint(0, 1), "SLOTS": rnd.randint(0, 20)}[name]
    return tune


def random_shapes(seed, n):
    """(frames, tile_count, trace_bpf, spp, tune, cus, in_flight): trace_bpf * frames runs from 1 to the C2 count, small launches more often than large."""
    rnd = random.Random(seed)
    for i in range(n):
        frames, tile_count = rnd.choice(FRAMES), rnd.choice(TILE_COUNTS)
        top = max(1, C2_BATCHES // frames)
        bpf = 1 if i % 17 == 0 else (top if i % 17 == 1 else max(1, min(top, int(round(2.0 ** rnd.uniform(0.0, np.log2(top)))))))
        spp = rnd.choice([s for s in range(1, 65) if bpf % s == 0])
        yield frames, tile_count, bpf, spp, random_tune(rnd), rnd.choice((CUS, CUS, CUS, 1, 8)), rnd.choice((0, 0, 1, 5))


def check_clamps(p, what):
    assert p["chunk_items"] % 64 == 0 and p["chunk_items"] >= 64, what
    assert 1 <= p["perm_rows"] <= 4096, what
    assert 1 <= p["slots"] <= K_MAX_SLOTS and p["slots"] <= p["setup_slots"] <= K_MAX_SLOTS, what
    assert p["grid"] >= 1, what
    assert p["total_items"] == p["perm_rows"] * p["perm_cols"] * 64 < qm.U32, what
    assert p["quad_live"] <= 16, what
    if p["xcd_span"]:
        assert p["xcd_span"] % p["chunk_items"] == 0 and 8 * p["xcd_span"] >= p["total_items"], what


def check_ranges(L, what):
    """The device computes a range's bounds (qi * span, that + span) in 32 bits: they have to be the exact ones."""
    for qi in range(8 if L.span else 0):
        assert qi * L.span + L.span < qm.U32, (what, qi)


def check_cover(L, num_batches, rnd, wave_sets, what):
    """Exact-once cover under seeded claim orders, and the model's closed count of cursor adds against the simulated one."""
    check_ranges(L, what)
    for xcds in wave_sets:
        got, Q = qm.drain(L, xcds, rnd)
        assert all(Q.dry), what
        got.sort()
        at = 0
        for first, last in got:                                  # the claimed ranges tile [0, total): nothing twice, nothing left out
            assert first == at and last > first and first % 64 == 0 and last % 64 == 0, (what, first, last, at)
            at = last
        assert at == L.total, what
        assert [Q.cursor(k) for k in range(len(Q.rng))] == qm.final_cursors(L, len(xcds)), what
        assert max(Q.cursor(k) for k in range(len(Q.rng))) <= qm.U32 - 1, what
    q = qm.decode_batches(L, 0, L.total // 64)
    valid = q < np.uint64(num_batches)
    assert int(valid.sum()) == num_batches, what                 # ... and behind the logical batches: every real batch ...
    assert np.array_equal(np.sort(q[valid]), np.arange(num_batches, dtype=np.uint64)), what      # ... exactly once; the others are padding
    assert int((~valid).sum()) == L.total // 64 - num_batches, what


def test_every_plan_under_overrides_hands_out_every_batch_once_and_ends():
    rnd = random.Random(20260402)
    refused = made = xcd_plans = padded = 0
    for frames, tile_count, bpf, spp, tune, cus, in_flight in random_shapes(11, 220):
        batches = bpf * frames
        what = dict(frames=frames, tile_count=tile_count, trace_bpf=bpf, spp=spp, tune=tune, cus=cus, in_flight=in_flight)
        p, err = plan_or_refusal(frames, tile_count, batches, tune, cus, in_flight)
        if p is None:
            assert err in REFUSALS, (what, err)
            refused += 1
            continue
        made += 1
        what["plan"] = p
        check_clamps(p, what)
        L = qm.Launch(p, batches, bpf, spp)
        waves = p["grid"] * WAVES_PER_GROUP
        check_ranges(L, what)
        # no cursor wraps with the launch's own number of wavefronts (the closed count; the drains below check that count against simulated adds)
        assert max(qm.final_cursors(L, waves)) <= qm.U32 - 1, what
        if L.total // L.chunk + 9 * waves > 60000:              # (drains of this many claims are left to the closed count)
            continue
        xcd_plans += 1 if L.span else 0
        padded += 1 if L.total // 64 > 2 * batches else 0
        few = min(rnd.randint(2, 40), waves)                      # (never more wavefronts than the launch has: the cursor guard is for ITS grid)
        wave_sets = [[rnd.randrange(8)], [rnd.randrange(8) for _ in range(waves)], [rnd.randrange(8)] * few, [rnd.randrange(8) for _ in range(few)]]
        check_cover(L, batches, rnd, wave_sets, what)
    assert made >= 150 and refused >= 5 and xcd_plans >= 30 and padded >= 10, (made, refused, xcd_plans, padded)      # the generator reaches what it is meant to


def test_the_launch_shapes_small_frames_never_reach():
    """One plan per branch of plan_launch that the small GPU frames leave out, by name."""
    rnd = random.Random(3)
    cases = {
        "xcd on by default (work8 >= 64)": (9, 1, 5, {}, lambda p: p["xcd_span"] != 0),
        "one row per frame": (5, 1, 7, {}, lambda p: p["perm_rows"] == 5),
        "three slots": (32, 1, 3, {}, lambda p: p["slots"] == 3),
        "four slots": (8, 1, 3, {}, lambda p: p["slots"] == 4),
        "grid divisor of an eighth share": (1, 8, 40, {}, lambda p: p["grid"] == CUS * 24 // WAVES_PER_GROUP // 4),
        "padding exceeds the real batches": (3, 1, 2, {"ROWS": 4096}, lambda p: p["perm_rows"] * p["perm_cols"] > 2 * 6),
        "empty xcd ranges": (1, 1, 1, {"XCD": 1, "ROWS": 1}, lambda p: p["xcd_span"] >= p["total_items"]),
        "far more wavefronts than chunks": (1, 1, 2, {"GRIDDIV": 1}, lambda p: p["grid"] > 50 * (p["total_items"] // p["chunk_items"])),
        "far fewer wavefronts than chunks": (9, 1, 500, {"GRIDDIV": 0xFFFFFFFE, "CHUNK": 64}, lambda p: p["grid"] == 1 and p["total_items"] // 64 >= 4500),
    }
    for name, (frames, tile_count, bpf, tune, holds) in cases.items():
        p, err = plan_or_refusal(frames, tile_count, bpf * frames, tune)
        assert p is not None and holds(p), (name, p, err)
        check_clamps(p, name)
        L = qm.Launch(p, bpf * frames, bpf)
        waves = p["grid"] * WAVES_PER_GROUP
        check_cover(L, bpf * frames, rnd, [[0], [rnd.randrange(8) for _ in range(waves)], [5] * min(7, waves)], name)


def test_xcd_ranges_at_chunks_near_the_cursor_guard():
    """A one-wavefront grid lets chunks of up to 2^31 items past the cursor guard; eight ranges of such a span do not fit 32 bits, and a range
    whose first item wrapped to 0 would hand the launch's items out again.  Such a plan has to fall back to one cursor (or be refused)."""
    rnd = random.Random(4)
    made = 0
    for cus, griddiv in ((1, 0xFFFFFFFE), (1, 12), (1, 8), (256, 0xFFFFFFFE), (256, 3000)):
        for shift in range(20, 32):
            for batches in (1, 9, 5000):
                tune = {"GRIDDIV": griddiv, "CHUNK": 1 << shift, "XCD": 1, "ROWS": rnd.choice((1, 3, 64))}
                p, err = plan_or_refusal(1, 1, batches, tune, cus)
                if p is None:
                    assert err in REFUSALS, (tune, err)
                    continue
                made += 1
                check_clamps(p, tune)
                waves = p["grid"] * WAVES_PER_GROUP
                L = qm.Launch(p, batches, batches)
                assert max(qm.final_cursors(L, waves)) <= qm.U32 - 1, (tune, p)
                check_cover(L, batches, rnd, [[rnd.randrange(8) for _ in range(waves)]], (tune, p))
    assert made >= 60, made


def test_refusals_stay_refusals():
    for frames, batches, tune in ((256, 0x03FFFFF0, {}), (1, 0x04000000, {"ROWS": 1}), (1, 4096, {"CHUNK": 1 << 31}), (1, 1 << 20, {"CHUNK": 1 << 20}),
                                  (1, 64, {"CHUNK": 0xFFFFFFC0, "GRIDDIV": 0xFFFFFFFE})):
        p, err = plan_or_refusal(frames, 1, batches, tune)
        assert p is None and err in REFUSALS, (frames, batches, tune, p, err)
    with pytest.raises(rt.PtError):
        rt.debug_launch_plan_tuned(CUS, 1, 1, 0, 1, 1, {"NOSUCHKNOB": 1})
    # no override at all: the defaults' plan, field for field
    import ctypes as C
    out = (C.c_uint32 * 12)()
    assert rt.lib.pt_debug_launch_plan(C.c_uint32(CUS), C.c_uint32(20), C.c_uint32(1), C.c_uint32(0), C.c_uint32(20 * C2_BATCHES), C.c_uint32(20), out) == 0
    assert rt.debug_launch_plan_tuned(CUS, 20, 1, 0, 20 * C2_BATCHES, 20, {}) == dict(zip(rt.PLAN_FIELDS, out))


def test_magic_division_is_exact_for_every_divisor_a_plan_can_produce():
    top_lb = (1 << 26) - 1                                       # total_items < 2^32: fewer than 2^26 logical batches
    divisors = set(range(1, 4097)) | {C2_BATCHES, C2_BATCHES // 4, 240, 135, 240 * 135, 240 * 135 * 64, 4095 * 64, (1 << 26) - 1, 1 << 26, (1 << 31) + 1, qm.U32 - 1}
    for d in sorted(divisors):
        m = qm.magic_of(d)
        assert m == (0xFFFFFFFF if d == 1 else (1 << 32) // d)
        for n in {0, d - 1, d, d + 1, 2 * d - 1, 2 * d, top_lb - 1, top_lb, top_lb // d * d, max(top_lb // d * d - 1, 0), qm.U32 - 1, (qm.U32 - 1) // d * d, max((qm.U32 - 1) // d * d - 1, 0)}:
            if n < qm.U32:
                assert qm.divmod_magic(n, d, m) == divmod(n, d), (n, d)
    rnd = random.Random(9)
    for d in list(range(1, 65)) + [rnd.randint(1, 4096) for _ in range(60)]:
        n = np.array([rnd.randrange(qm.U32) for _ in range(500)] + [0, d - 1, d, qm.U32 - 1], np.uint64)
        q, r = qm.divmod_magic_np(n, d)
        assert np.array_equal(q, n // np.uint64(d)) and np.array_equal(r, n % np.uint64(d)), d


def test_item_decoding_reaches_every_pixel_sample_of_every_traced_tile_once():
    """The scalar decode, item by item, on launches small enough to enumerate: ragged frames, a list of traced tiles, several samples and frames."""
    rnd = random.Random(77)
    for case in range(14):
        frames, spp = rnd.choice((1, 2, 3, 5, 9)), rnd.choice((1, 2, 3, 5))
        tiles_x, tiles_y = rnd.randint(1, 6), rnd.randint(1, 4)
        width, height = tiles_x * 8 - rnd.randint(0, 7), tiles_y * 8 - rnd.randint(0, 7)
        traced = sorted(rnd.sample(range(tiles_x * tiles_y), rnd.randint(1, tiles_x * tiles_y)))
        bpf = len(traced) * spp
        tune = {"ROWS": rnd.choice((1, 2, 7, frames, 64, 4096)), "CHUNK": rnd.choice((64, 128, 192)), "XCD": rnd.randint(0, 1)}
        p, err = plan_or_refusal(frames, 1, bpf * frames, tune)
        assert p is not None, err
        L = qm.Launch(p, bpf * frames, bpf, spp, tiles_x, width, height, traced)
        seen = {}
        for item in range(L.total):
            d = qm.decode(L, item)
            if d is not None:
                frame, tslot, s, pp, px, py = d
                key = (frame, px, py, s)
                assert key not in seen, (case, item, seen[key])
                seen[key] = item
                assert traced[tslot] == (py // 8) * tiles_x + px // 8 and pp == (py % 8) * 8 + px % 8
        want = {(f, x, y, s) for f in range(frames) for s in range(spp) for t in traced
                for y in range(t // tiles_x * 8, min(t // tiles_x * 8 + 8, height)) for x in range(t % tiles_x * 8, min(t % tiles_x * 8 + 8, width))}
        assert set(seen) == want, case


def test_thresholds_that_are_not_clamped_and_the_one_that_is():
    """SHADE, FILL and FORK reach the kernel as they are set: its passes also fire when nothing traverses, and FORK is only compared with 0 and 2
    (tests/knob_lattice.py::WHY).  QUAD is the one the kernel could not take as it comes -- a wavefront has sixteen quads -- and is clamped."""
    for v in (0, 1, 16, 17, 64, 65, 0x10000, 0xFFFFFFFE):
        p, err = plan_or_refusal(3, 1, 40, {"SHADE": v, "FILL": v, "FORK": v, "QUAD": v})
        assert p is not None, err
        assert (p["shade_threshold"], p["fill_threshold"], p["fork_shadow"], p["quad_live"]) == (v, v, v, min(v, 16))
    p, _ = plan_or_refusal(3, 1, 40, {})
    assert (p["shade_threshold"], p["fill_threshold"], p["fork_shadow"], p["quad_live"]) == (16, 4, 2, 16)


def test_the_lattice_shapes_are_what_they_are_meant_to_be():
    """The oracle's own view of the lattice's scenes and cameras: from outside the object stands in front of background, from inside every ray enters the
    tree, from beside nothing is hit; and no two frames of a row are the same image, in any mode."""
    import orc as orc_mod
    orc = orc_mod.load()
    for scene, (kind, n) in kl.SCENES.items():
        tris = rt.procedural_scene(kind, n)
        _, bvh4 = orc.build_bvh4(tris)
        for cam in kl.FACTORS["camera"]:
            frames = []
            for i in (0, 1, 8):
                pos, quat = kl.frame_camera({"camera": cam}, i)
                img, ids, st = orc.render(orc.make_params(97, 61, n, pos, quat, mode=orc_mod.MODE_SINGLE), tris, bvh4, want_tri_ids=True)
                hit = float((ids != 0xFFFFFFFF).mean())
                if cam == "beside":
                    assert hit == 0.0 and st["nodes_examined"] == st["rays_closest"], (scene, cam, hit)      # one root record per ray, nothing entered
                elif cam == "inside":
                    assert hit > 0.5 and st["nodes_examined"] > 4 * st["rays_closest"], (scene, cam, hit)          # (the root box is entered by every ray: its children are examined)
                else:
                    assert 0.1 < hit and (scene != "object" or hit < 0.7), (scene, cam, hit)
                frames.append(img)
            if cam != "beside":
                assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2]), (scene, cam)
    assert all(sum(c * c for c in kl.FAR_CAMERA) >= sum(c * c for c in kl.frame_camera({"camera": cam}, i)[0]) for cam in kl.CAMERAS for i in range(9))


def test_the_lattice_rows_cover_every_pair_of_levels():
    for scene in kl.SCENES:
        rows = kl.pairwise_rows(scene)
        assert len(rows) <= kl.MAX_PAIRWISE_ROWS, len(rows)
        assert rows == kl.pairwise_rows(scene)                   # deterministic
        names = list(kl.FACTORS)
        for a, b in itertools.combinations(names, 2):
            want = {(x, y) for x in kl.FACTORS[a] for y in kl.FACTORS[b] if kl.allowed(a, x, b, y)}
            have = {(r[a], r[b]) for r in rows}
            assert want <= have, (scene, a, b, sorted(want - have, key=repr))
        for r in rows:
            assert set(r) == set(names) and all(r[k] in kl.FACTORS[k] for k in names)
    single = kl.one_at_a_time_rows()
    for name, levels in kl.FACTORS.items():
        assert {r[name] for r in single} == set(levels), name
    assert len(single) == 1 + sum(len(v) - 1 for v in kl.FACTORS.values())
    queue = kl.queue_rows()
    assert len(queue) == len(set(map(repr, queue))) == np.prod([len(kl.FACTORS[k]) for k in kl.QUEUE_FACTORS]) * len(kl.QUEUE_SHAPES)
    assert not kl.EXCLUDED_PAIRS                                  # every pair of levels is allowed: nothing is carved out of the lattice
    for name, levels in kl.FACTORS.items():                      # every level has its line on why a launch with it ends
        for lv in levels:
            assert len(kl.WHY[name][lv]) >= 12, (name, lv)
