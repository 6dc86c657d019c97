"""The knob lattice on the GPU (tests/knob_lattice.py): a setting of the fifteen PtTune knobs, of the launch kind, the submission, the tile share
and the frame's shape changes no bit of a frame -- every frame of every row equals the CPU oracle's, rendered over the context's read-back BVH4;
on instrumented rows the counters are the oracle's too.  The oracle's frames are computed once per (scene, camera, frame, shape) and shared.

Every row runs on one context per test function, sets its knobs through debug_set_tune and restores them; the assertion message carries the
whole row.  Rows with an instrumented launch run a second time as production launches: the two kinds trace different tile sets (an
instrumented launch keeps the root box's rectangle) and have to give the same image."""
import ctypes as C
import time

import numpy as np
import pytest

import knob_lattice as kl
import orc as orc_mod

pytestmark = pytest.mark.gpu

COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "samples", "max_stack", "stack_drops")
MODES = {"packet": (0, orc_mod.MODE_PACKET), "single": (1, orc_mod.MODE_SINGLE), "path": (2, orc_mod.MODE_PATH)}
BUF_FLOATS = 32768 * 4              # one frame of the largest resolution (200 x 120), whole or as a compact share with its padded edge tiles
_oracle_frames = {}                 # (scene, camera, frame, mode, spp, res) -> (image, counters): computed once, never written to


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def says(**kw):
    """The assertion message: the whole row, as text (pytest abbreviates a dict)."""
    return repr(kw)


class Rig:
    """One context with the scene's tree, nine device buffers for the frames of a launch, and the oracle's view of the same tree."""

    def __init__(self, rt, orc, ctx, scene):
        self.rt, self.orc, self.ctx, self.scene = rt, orc, ctx, scene
        self.tris = rt.procedural_scene(*kl.SCENES[scene])
        ctx.set_triangles(self.tris); ctx.build_bvh()
        self.bvh4 = ctx.read_bvh4()
        self.hip = C.CDLL("libamdhip64.so")
        self.bufs = []
        for _ in range(max(kl.FACTORS["frames"])):
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), C.c_size_t(BUF_FLOATS * 4)) == 0
            self.bufs.append(p)
        self.launches = 0

    def close(self):
        for b in self.bufs:
            self.hip.hipFree(b)

    def oracle(self, row, i):
        spp = row["spp"] if row["mode"] == "path" else 1
        key = (self.scene, row["camera"], i, row["mode"], spp, row["res"])
        if key not in _oracle_frames:
            (w, h), (pos, quat) = row["res"], kl.frame_camera(row, i)
            p = self.orc.make_params(w, h, self.tris.size // 9, pos, quat, mode=MODES[row["mode"]][1], spp=spp, max_bounces=kl.MAX_BOUNCES, seed=kl.SEED, frame=i)
            img, _, st = self.orc.render(p, self.tris, self.bvh4)
            img.setflags(write=False)
            _oracle_frames[key] = (img, st)
        return _oracle_frames[key]

    def params(self, row, i, stats):
        (w, h), (pos, quat), (count, rank) = row["res"], kl.frame_camera(row, i), row["share"]
        return self.ctx.make_params(w, h, pos, quat, mode=MODES[row["mode"]][0], spp=row["spp"], max_bounces=kl.MAX_BOUNCES, seed=kl.SEED, frame=i,
                                    tile_rank=rank, tile_count=count, stats=stats)

    def read(self, i, floats):
        host = np.zeros(floats, np.float32)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.bufs[i], C.c_size_t(floats * 4), 2) == 0
        return host

    def expected_share(self, row, img):
        """The oracle's frame in the compact layout of the row's tile share: 64 pixels per owned tile, tile after tile in pt_tile_ids order, pixel p of
        a tile at (p & 7, p >> 3); -> (values, which of them lie inside the frame)."""
        (w, h), (count, rank) = row["res"], row["share"]
        ids = self.rt.tile_ids(w, h, rank, count).astype(np.int64)
        tiles_x = (w + 7) // 8
        p = np.arange(64)
        px = (ids % tiles_x)[:, None] * 8 + (p & 7)[None, :]
        py = (ids // tiles_x)[:, None] * 8 + (p >> 3)[None, :]
        inside = (px < w) & (py < h)
        vals = np.zeros((len(ids), 64, 4), np.float32)
        vals[inside] = img[py[inside], px[inside]]
        return vals, inside

    def run(self, row):
        ctx, F, sharded = self.ctx, row["frames"], row["share"][0] > 1
        passes = (False,) if row["stats"] == "off" else (True, False)         # an instrumented row also runs as production launches: the same image either way
        for k, v in kl.tune_of(row).items():
            ctx.debug_set_tune(k, v)
        try:
            for stats in passes:
                if row["EXPOSE"] != 0:                                            # the mask of this row's budget, for a camera at least as far as every frame's
                    ctx.debug_exposure(ctx.make_params(row["res"][0], row["res"][1], kl.FAR_CAMERA, mode=2, spp=1), want_mask=False)
                ctx.set_batch(F if row["submit"] == "batched" else 1)
                for i in range(F):                                                # no host wait between the frames in either submission
                    if sharded:
                        ctx.set_compact_buffer(self.bufs[i].value, BUF_FLOATS)
                    else:
                        ctx.set_output_buffer(self.bufs[i].value, BUF_FLOATS)
                    ctx.render(self.params(row, i, stats))
                ctx.flush(); ctx.synchronize()
                self.launches += F if (row["submit"] == "nowait" or row["mode"] == "packet" or (stats and row["stats"] == "on")) else 1
                w, h = row["res"]
                for i in range(F):
                    want, _ = self.oracle(row, i)
                    if sharded:
                        vals, inside = self.expected_share(row, want)
                        got = self.read(i, vals.size).reshape(vals.shape)
                        same = np.array_equal(bits(got)[inside], bits(vals)[inside])
                    else:
                        got = self.read(i, w * h * 4).reshape(h, w, 4)
                        same = np.array_equal(bits(got), bits(want))
                    assert same, says(scene=self.scene, frame=i, instrumented=stats, row=row)
                if stats and not sharded:                                         # (a share's counters are a part of the frame's: the oracle has the whole frame's)
                    self.check_counters(row, ctx.stats())
        finally:
            for k in kl.tune_of(row):
                ctx.debug_set_tune(k, None)
            ctx.set_batch(1); ctx.set_output_buffer(0, 0); ctx.set_compact_buffer(0, 0)

    def check_counters(self, row, st):
        """The counters of the last instrumented launch: its last frame's, or with STATSBATCH in a batch all the frames' sums (max_stack: maximum)."""
        F = row["frames"]
        joined = row["stats"] == "on+STATSBATCH" and row["submit"] == "batched" and row["mode"] != "packet"
        frames = range(F) if joined else (F - 1,)
        want = {k: 0 for k in COUNTERS}
        for i in frames:
            ost = self.oracle(row, i)[1]
            for k in COUNTERS:
                want[k] = max(want[k], ost[k]) if k == "max_stack" else want[k] + ost[k]
        keys = COUNTERS
        if row["EXPOSE"] == 2 and row["mode"] == "path":
            # instrumented launches skip the shadow rays of exposed triangles as well: counted, and absent from the traversal counters
            skipped = self.ctx.debug_exposure(None, want_mask=False)["skipped"]
            assert st["rays_shadow"] + skipped == want["rays_shadow"], says(scene=self.scene, skipped=skipped, got=st, want=want, row=row)
            assert st["nodes_examined"] <= want["nodes_examined"] and st["tris_tested"] <= want["tris_tested"], says(scene=self.scene, got=st, want=want, row=row)
            keys = ("rays_closest", "samples", "stack_drops") if skipped else COUNTERS
        for k in keys:
            assert st[k] == want[k], says(scene=self.scene, counter=k, got=st[k], want=want[k], row=row)


def run_rows(rt, orc, ctx, scene, rows, label):
    """Runs the rows in order on one context and prints their count, the launches and the wall time (the oracle's frames of a new camera, frame or
    shape are part of the first row that needs them)."""
    t0 = time.time()
    rig = Rig(rt, orc, ctx, scene)
    try:
        for row in rows:
            rig.run(row)
    finally:
        rig.close()
    print("%s: %d rows, %d launches, %.2f s" % (label, len(rows), rig.launches, time.time() - t0))


def test_the_beside_camera_leaves_nothing_to_trace(rt, gpu_ctx):
    """What the lattice's third camera is for: the root box's rectangle is empty, so every queue knob meets total_items == 0."""
    for scene in kl.SCENES:
        gpu_ctx.set_triangles(rt.procedural_scene(*kl.SCENES[scene])); gpu_ctx.build_bvh()
        for i in (0, 8):
            pos, quat = kl.frame_camera({"camera": "beside"}, i)
            for w, h in kl.FACTORS["res"]:
                _, rect_tiles, traced = gpu_ctx.debug_traced_tiles(gpu_ctx.make_params(w, h, pos, quat, mode=rt.PT_MODE_PATH, spp=1))
                assert rect_tiles == 0 and traced == 0, (scene, i, w, h)
        pos, quat = kl.frame_camera({"camera": "outside"}, 0)
        mask, rect_tiles, _ = gpu_ctx.debug_traced_tiles(gpu_ctx.make_params(200, 120, pos, quat, mode=rt.PT_MODE_PATH, spp=1))
        assert 0 < rect_tiles and (scene != "object" or rect_tiles < mask.size), (scene, rect_tiles)      # the object stands in front of culled background tiles


@pytest.mark.parametrize("scene", sorted(kl.SCENES))
def test_every_level_alone_is_bit_identical_to_the_oracle(rt, orc, gpu_ctx, scene):
    rows = kl.one_at_a_time_rows()
    run_rows(rt, orc, gpu_ctx, scene, rows, "one at a time, %s" % scene)


@pytest.mark.parametrize("shape", sorted(kl.QUEUE_SHAPES))
def test_the_queue_knobs_in_full_are_bit_identical_to_the_oracle(rt, orc, gpu_ctx, shape):
    rows = kl.queue_rows(shape)
    run_rows(rt, orc, gpu_ctx, "object", rows, "queue subset, %s" % shape)


@pytest.mark.parametrize("scene", sorted(kl.SCENES))
def test_every_pair_of_levels_is_bit_identical_to_the_oracle(rt, orc, gpu_ctx, scene):
    rows = kl.pairwise_rows(scene)
    run_rows(rt, orc, gpu_ctx, scene, rows, "pairwise, %s" % scene)
