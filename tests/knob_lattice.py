"""The knob lattice of tests/test_gpu_knob_lattice.py: factors, their levels, why a launch with each level still ends, and the rows -- no GPU here.

DESIGN.md section 6.1: a knob of PtTune changes WHEN work happens, never WHAT is computed.  So every row -- one setting of every factor -- must
give the CPU oracle's frames bit for bit.  Three kinds of rows: every level of every factor with the rest at their base level
(one_at_a_time_rows), the queue's own knobs in full (queue_rows), and a covering array in which every pair of levels of every two factors
occurs at least once (pairwise_rows; checked without a GPU by tests/test_queue_model.py::test_the_lattice_rows_cover_every_pair_of_levels).

A level None leaves the knob at 0xFFFFFFFF, the measured default.  Before a value went in, its consumer was read (pt_api.cpp::plan_launch,
pt_megakernel.hip, pt_megakernel_loop.inc): WHY holds one line per level on why a launch with it ends.  Common to all of them: a wavefront
leaves its loop when nothing traverses, nothing waits for a shade pass and the source is dry; a claim always advances a cursor, so the source
runs dry after finitely many claims; the shade pass and the refill pass also fire whenever NOTHING traverses (`m_trav == 0`), whatever their
thresholds say."""
import itertools
import random

SCENES = {"object": (0, 2000), "interior": (1, 12000)}      # procedural_scene(kind, triangles): an object in front of background (culled tiles); an interior at its smallest size

# camera position, quaternion (x, y, z, w).  "beside" stands six units to the right and looks past the scene: all of the root box is in front of the eye and left of the image, its rectangle holds no tile (total_items == 0 under every queue knob)
CAMERAS = {"outside": ((0.0, 0.0, 2.5), (0.0, 0.0, 0.0, 1.0)), "inside": ((0.1, 0.05, 0.1), (0.0, 0.0, 0.0, 1.0)), "beside": ((6.0, 0.0, 2.5), (0.0, 0.0, 0.0, 1.0))}
FAR_CAMERA = (6.2, 0.0, 2.5)                                 # at least as far from the origin as every frame's camera: what the exposure mask is primed for
FRAME_STEP = 0.02                                            # frame i of a row stands FRAME_STEP * i to the right: no two frames of a launch are the same image in any mode
MAX_BOUNCES, SEED = 4, 3

FACTORS = {
    "GRIDDIV": (None, 1, 1024),
    "ROWS": (None, 1, 7, "frames", 4096),
    "CHUNK": (None, 64, 192, 512, 4096),
    "XCD": (None, 0, 1),
    "SHADE": (None, 0, 1, 64),
    "FILL": (None, 0, 1, 64),
    "SLOTS": (None, 1, 2, 16),
    "QUAD": (0, 1, 5, 16),
    "FORK": (0, 1, 2),
    "BOUNDED": (0, 1),
    "CULL": (0, 1, 2),
    "EXPOSE": (0, 1, 2),
    "EXBUDGET": (None, 0),
    "TIMELINE": (0, 1),
    "stats": ("off", "on", "on+STATSBATCH"),
    "frames": (1, 3, 9),
    "submit": ("batched", "nowait"),
    "share": ((1, 0), (2, 1), (8, 5)),
    "mode": ("packet", "single", "path"),
    "res": ((8, 8), (97, 61), (200, 120)),
    "spp": (1, 3),
    "camera": ("outside", "inside", "beside"),
}
KNOBS = ("GRIDDIV", "ROWS", "CHUNK", "XCD", "SHADE", "FILL", "SLOTS", "QUAD", "FORK", "BOUNDED", "CULL", "EXPOSE", "EXBUDGET", "TIMELINE")

# the row everything else is varied from: every knob at (or equal to) its default
BASE = {"GRIDDIV": None, "ROWS": None, "CHUNK": None, "XCD": None, "SHADE": None, "FILL": None, "SLOTS": None, "QUAD": 16, "FORK": 2, "BOUNDED": 1, "CULL": 2,
        "EXPOSE": 1, "EXBUDGET": None, "TIMELINE": 0, "stats": "off", "frames": 3, "submit": "batched", "share": (1, 0), "mode": "path", "res": (97, 61), "spp": 3,
        "camera": "outside"}

WHY = {
    "GRIDDIV": {
        None: "the measured divisor: the grid every existing test launches",
        1: "the whole grid, far more wavefronts than chunks: a wavefront whose first claim is past total_items is told `dry`, holds no lane in flight and leaves at once",
        1024: "divided by the frame count and floored at 1 in plan_launch, the grid rounded up: at least one workgroup; its wavefronts claim chunk after chunk and each claim advances the cursor",
    },
    "ROWS": {
        None: "the measured row count",
        1: "one row: perm_cols = num_batches, q = pcol, no padding, the batches in their own order",
        7: "up to six padded batches: q >= num_batches makes all 64 items invalid, no ray is stored and the refill loop goes on to the next batch or finds the queue dry",
        "frames": "one row per frame (what long launches take by default), here on a short one: rows divide the batch count, no padding",
        4096: "the clamp's upper bound, more padding than work on these frames: padded batches are decoded, found invalid and skipped 64 items at a time; total_items stays far below the cursor guard",
    },
    "CHUNK": {
        None: "the measured two batches per claim",
        64: "one batch per claim: the smallest chunk the clamp allows; chunk_next reaches chunk_end after one batch",
        192: "three batches, no power of two: rounded to itself by (chunk + 63) / 64 * 64; ranges end on min(start + chunk, end) and all bounds are multiples of 64, so chunk_next meets chunk_end exactly",
        512: "eight batches per claim; the XCD span is rounded up to whole chunks, a range's last claim is cut at the range's end",
        4096: "64 batches per claim, more than these launches hold: the first claim takes everything, the cursor guard (total + (waves + 1) * chunk < 2^32) holds by a factor of 100",
    },
    "XCD": {
        None: "the measured rule: eight cursors from 8 frames of work on (frames = 9), one below",
        0: "one cursor: a claim at or past total_items ends the wavefront's source",
        1: "eight cursors on launches of a few batches: ranges past total_items are empty (q_begin >= q_end), a wavefront hops over them and is dry after eight dry ranges",
    },
    "SHADE": {
        None: "the measured 16 lanes",
        0: "`done >= 0` always holds: the inner loop returns after every traversal step, a shade pass runs whenever a lane is done; each outer round still makes one step",
        1: "a shade pass as soon as one lane is done",
        64: "a full wavefront of done lanes is rare: the pass then fires through `m_trav == 0`, when nothing traverses any more, and after the queue is dry through shade_due's quarter of the live lanes",
    },
    "FILL": {
        None: "the measured 4 lanes",
        0: "`idle >= 0` always holds: the inner loop returns after every step and a refill runs whenever a lane is idle and the source is not dry; a dry source sets the threshold to 0x10000",
        1: "a refill as soon as one lane is idle",
        64: "only a wavefront with all lanes idle reaches it: otherwise the refill fires through `m_trav == 0`, when nothing traverses",
    },
    "SLOTS": {
        None: "the measured count for the launch's size",
        1: "one slot: every launch waits for the resolve of the one before it (the slot's `resolved` event); nothing overlaps",
        2: "two slots in rotation",
        16: "kMaxSlots, the clamp's upper bound in slots_for: sixteen side streams, each slot with buffers of its own",
    },
    "QUAD": {
        0: "never re-seats: the one-ray-per-lane loop runs to the end, as before quad mode existed",
        1: "re-seats when a single path is left",
        5: "re-seats at five paths or fewer: eleven quads stay free for forked shadow rays",
        16: "the default and the clamp (min(16, .)): sixteen paths, one per quad of a wavefront",
    },
    "FORK": {
        0: "no shadow ray is handed over: a path traces its own, as the oracle orders them",
        1: "handed to idle quads only (quad mode); a path without an idle seat traces its shadow ray itself",
        2: "the default: idle lanes take shadow rays as soon as the source is dry (the loop's second instance starts nothing new, so it ends when its paths do)",
    },
    "BOUNDED": {
        0: "the general reciprocal and square root: another kernel variant, the same control flow",
        1: "the default: the short forms where the host has bounded their operands",
    },
    "CULL": {
        0: "every owned tile is traced, no list of traced tiles",
        1: "the root box's rectangle; a camera that sees none of it gives num_batches == 0, total_items == 0: launch_trace starts no kernel, the resolve pass delivers the miss values",
        2: "the default: the tile cover inside the rectangle (taken once a view repeats); instrumented and TIMELINE launches keep the rectangle",
    },
    "EXPOSE": {
        0: "every shadow ray is traced",
        1: "the default: production launches skip the shadow rays of exposed triangles, the term is added in the shade pass: fewer rays, no new wait",
        2: "instrumented launches skip them too; the counters then differ from the oracle's by the skipped rays, which are counted",
    },
    "EXBUDGET": {
        None: "the measured leaf budget of the exposure pass",
        0: "every query of the exposure pass that reaches a leaf gives up at once: a shorter pass, an empty mask, every shadow ray traced",
    },
    "TIMELINE": {
        0: "the production kernel",
        1: "the TIMELINE variant: the production kernel plus wave-uniform counts and four event records; keeps the rectangle like an instrumented launch",
    },
    "stats": {
        "off": "the production kernel",
        "on": "the COUNTERS variant, one launch per frame in slot 0, never overlapped",
        "on+STATSBATCH": "STATSBATCH = 1: the instrumented frames of a batch join one launch (tools/wave_timeline.py's use); the counters are the launch's sums",
    },
    "frames": {
        1: "one frame per launch",
        3: "three frames: the grid divisor is divided by the frame count",
        9: "nine frames: 72 eighths of a frame of work, the XCD-aware queue is on by default and rows = frames",
    },
    "submit": {
        "batched": "pt_set_batch(frames): one launch, written when the batch is full",
        "nowait": "one render() per frame with no host wait between them: launches rotate through the frame slots and shrink their grid with the launches in flight",
    },
    "share": {
        (1, 0): "the whole frame",
        (2, 1): "every second tile: a tile list, compact output; a one-tile frame leaves rank 1 nothing (num_tiles == 0: neither the trace nor the resolve kernel is launched)",
        (8, 5): "an eighth of the tiles, grid / 4; a share without a tile launches nothing",
    },
    "mode": {
        "packet": "the 2 x 2 packet kernel: not the megakernel, one thread per packet, no queue -- the knobs must not reach it",
        "single": "PT_MODE_REFERENCE on the megakernel: one ray per pixel, a miss frees its lane without a shade pass",
        "path": "the path tracer: shade passes, shadow rays, bounces",
    },
    "res": {
        (8, 8): "one tile: one batch per sample and frame, seven empty XCD ranges",
        (97, 61): "13 x 8 tiles with ragged right and bottom edges: items of edge tiles outside the frame are invalid",
        (200, 120): "25 x 15 tiles: more than one chunk per wavefront at small grids",
    },
    "spp": {
        1: "one sample: spp_magic is the d == 1 case of the magic division",
        3: "three samples per pixel: the sample index is part of the batch order",
    },
    "camera": {
        "outside": "in front of the scene: background tiles around it are culled",
        "inside": "inside the root box: every ray enters the tree, nothing is culled",
        "beside": "looks past the scene: every tile is culled unless CULL = 0 (total_items == 0: no trace kernel); the resolve pass delivers the primed miss values",
    },
}

# pairs of levels that cannot be run together: none.  (allowed() is what the coverage test and the generator share.)
EXCLUDED_PAIRS = ()


def allowed(a, x, b, y):
    return (a, x, b, y) not in EXCLUDED_PAIRS and (b, y, a, x) not in EXCLUDED_PAIRS


MAX_PAIRWISE_ROWS = 64      # two factors of five levels need 25 rows; a greedy array over 22 factors stays within about twice that.  A bound, so that the lattice cannot quietly grow either


def one_at_a_time_rows():
    rows = [dict(BASE)]
    for name, levels in FACTORS.items():
        for lv in levels:
            if lv != BASE[name]:
                r = dict(BASE); r[name] = lv
                rows.append(r)
    return rows


QUEUE_FACTORS = ("GRIDDIV", "ROWS", "CHUNK", "XCD", "frames")
QUEUE_SHAPES = {"8x8": {"res": (8, 8), "spp": 3}, "97x61": {"res": (97, 61), "spp": 1}}


def queue_rows(shape=None):
    """GRIDDIV x ROWS x CHUNK x XCD x frames in full, in path mode, on the one-tile frame and on the ragged one."""
    rows = []
    for name, over in QUEUE_SHAPES.items():
        if shape is not None and name != shape:
            continue
        for combo in itertools.product(*[FACTORS[k] for k in QUEUE_FACTORS]):
            r = dict(BASE); r.update(over); r.update(zip(QUEUE_FACTORS, combo))
            rows.append(r)
    return rows


def pairwise_rows(scene):
    """A covering array of strength two over FACTORS by a seeded greedy pass: every new row starts from a pair that is still uncovered and takes,
    factor by factor, the level that covers the most uncovered pairs with the levels already chosen; of 24 such candidates the best is kept."""
    rnd = random.Random("knob lattice / " + scene)
    names = list(FACTORS)
    uncovered = {(a, x, b, y) for a, b in itertools.combinations(names, 2) for x in FACTORS[a] for y in FACTORS[b] if allowed(a, x, b, y)}

    def gain(row):
        return sum(1 for a, b in itertools.combinations(names, 2) if a in row and b in row and (a, row[a], b, row[b]) in uncovered)

    rows = []
    while uncovered:
        seeds = sorted(uncovered, key=repr)
        best, best_gain = None, -1
        for _ in range(24):
            a, x, b, y = seeds[rnd.randrange(len(seeds))]
            row = {a: x, b: y}
            rest = [n for n in names if n not in row]
            rnd.shuffle(rest)
            for n in rest:
                scored = []
                for lv in FACTORS[n]:
                    if all(allowed(n, lv, m, row[m]) for m in row):
                        g = sum(1 for m in row if ((n, lv, m, row[m]) if names.index(n) < names.index(m) else (m, row[m], n, lv)) in uncovered)
                        scored.append((g, rnd.random(), lv))
                row[n] = max(scored, key=lambda t: t[:2])[2]
            g = gain(row)
            if g > best_gain:
                best, best_gain = row, g
        rows.append({n: best[n] for n in names})
        uncovered -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
    return rows


def tune_of(row):
    """The (knob, value) pairs of a row for pt_debug_set_tune; None = leave at the default."""
    t = {k: (row["frames"] if row[k] == "frames" else row[k]) for k in KNOBS}
    t["STATSBATCH"] = 1 if row["stats"] == "on+STATSBATCH" else None
    return t


def frame_camera(row, i):
    pos, quat = CAMERAS[row["camera"]]
    return (pos[0] + FRAME_STEP * i, pos[1], pos[2]), quat
