"""Seeded mixed-operation sessions over ONE long-lived context (tests/test_gpu_session.py, tests/test_session_model.py).

generate(seed, length) gives a list of operation records (plain dicts: one line each in the log); run() plays them against a model that holds
plain data only -- the current triangles as float32[9n] and the current BVH2 / BVH4 words as the host twins give them -- and, with
device=True, against one context that lives for the whole session.  Every expected value comes from the host twins (rt.*_bvh4, rt.refit_*,
rt.build_bvh2_ploc, rt.collapse_*), from occlusion_rays_host and from the oracle (orc.render, orc.trace_ray) over the MODEL's words, never
from the context under test, so every comparison is on every bit.  The one exception is bvh_cost, a float64 sum the device adds in another
order: it keeps the bound of tests/test_gpu_refit.py, numNodes4 * 2^-51 relative.

The query inputs are the ones of the case modules (closest_cases, crossing_cases, radius_cases, knn_cases, box_cases, hitlist_cases,
test_gpu_rayquery.random_rays), spoiled the way the existing tests spoil them (NaN, zero, negative t_max / r_max at fixed strides).

The device leg needs torch imported BEFORE the package (the torch routes; raytracer-public_amd/__init__.py _TORCH_FIRST), so it runs in a
process of its own, like the *_torch_cases.py modules:  python tests/session_model.py gpu SEED [STOP_AFTER]
and  python tests/session_model.py cpu SEED [STOP_AFTER]  replays the model alone (twins and oracle, no context)."""
import os
import sys
import time

if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "gpu":
    import torch      # first: libmi355pt then binds to torch's copy of the HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import box_cases as bc  # noqa: E402
import closest_cases as clc  # noqa: E402
import crossing_cases as cc  # noqa: E402
import hitlist_cases as hlc  # noqa: E402
import knn_cases as kc  # noqa: E402
import orc as orc_mod  # noqa: E402
from refit_cases import wave  # noqa: E402
from scenes import quat_yaw_pitch, random_soup  # noqa: E402
from test_gpu_rayquery import random_rays  # noqa: E402

SEEDS = (5, 17, 29)
LENGTH = 240
MISS = 0xFFFFFFFF
COUNTERS = ("rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")         # include/mi355pt.h PtStats
NO_COUNTERS = ("trace_closest", "trace_any", "occlusion", "hit_surfels", "signed_distance")    # no twin counts them (or no counting form): never drawn with stats
CAMS = [((0, 0, 2.5), (0, 0, 0, 1)), ((0.4, 0.3, 1.7), quat_yaw_pitch(0.2, -0.15)), ((-0.5, 0.2, 2.2), quat_yaw_pitch(-0.2, -0.05)),
        ((0.3, 0.2, 3.6), (0, 0, 0, 1)), ((0.0, -0.4, 2.0), quat_yaw_pitch(0.0, 0.2)), ((0.1, 0.1, 3.0), quat_yaw_pitch(0.03, -0.03))]
LARGE = dict(w=1024, h=512, spp=4, bounces=8)                     # 2^24 ray segments and more: the launch that takes the exposure mask
LARGE_CAMS = {"near": (0.3, 0.2, 2.5), "far": (0.3, 0.2, 6.0)}
N_SMALL = (1, 63, 64, 65)

# the query families, by the buffers they keep between their launches (pt_context.h): the ray / point walks share d_rq_queue, d_rq_spill,
# d_rq_hits, d_oc_surfels and d_cr_contain; the list queries d_rd_counts, d_rd_temp, d_rd_offsets and d_rd_entries.  (The host routes of
# both groups stage their records in d_rq_rays.)
RAY_FAMILIES = ["trace_closest", "trace_any", "closest_points", "occlusion", "hit_surfels", "count_hits", "contains", "signed_distance", "nearest_k"]
LIST_FAMILIES = ["radius_count", "radius_search", "radius_search_cap", "list_hits", "list_hits_sorted", "list_hits_cap", "box_count", "box_search"]
FAMILIES = RAY_FAMILIES + LIST_FAMILIES
GROUP = dict([(f, "ray") for f in RAY_FAMILIES] + [(f, "list") for f in LIST_FAMILIES])
STATE_OPS = ("set_triangles", "build_bvh", "update", "set_bvh2", "set_bvh4", "set_bvh4_wide", "set_batch", "flush", "set_stream", "refuse")
OBSERVATIONS = ("scene_info", "read_bvh4", "read_bvh2", "bvh_cost", "render", "render_shares", "accum_run", "batch_run", "views", "large", "query")
BATCH_EVENTS = ("flush", "update", "set_bvh4", "set_stream", "query", "refuse")       # what may arrive while frames are pending (batch_run)
REFUSALS = ("update_count", "build_accel_7", "query_2_32", "set_bvh2_truncated")


class SessionMismatch(AssertionError):
    pass


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.astype(np.int64)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ---- the generator ------------------------------------------------------------------------------------------------------------------

class _Gen:
    """Appends operation records and tracks what a record may rely on: whether the model holds a BVH2, the size of the open accumulation,
    the stream the context is on."""

    def __init__(self, rng):
        self.rng, self.ops = rng, []
        self.bvh2, self.accum_dims, self.stream = False, None, "own"

    def add(self, op, **kw):
        self.ops.append(dict(op=op, **kw))

    def i(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def pick(self, seq):
        return seq[self.i(0, len(seq) - 1)]

    def alternate(self, family, torch=None, kernel=None):
        """the host route or the torch route; the persistent kernel, the simple kernel or the counting one (where the family has counters
        that a twin gives): drawn call by call unless the layout fixes them"""
        kinds = 1 if family == "hit_surfels" else 2 if family in NO_COUNTERS else 3
        kernel = self.i(0, kinds - 1) if kernel is None else kernel % kinds
        return dict(torch=bool(self.i(0, 1)) if torch is None else torch, simple=kernel == 1, stats=kernel == 2)

    # -- state
    def set_triangles(self, scene):
        self.add("set_triangles", scene=scene)
        self.bvh2, self.accum_dims = False, None

    def build(self, accel=None):
        self.add("build_bvh", accel=self.i(0, 2) if accel is None else accel)
        self.bvh2, self.accum_dims = True, None

    def update(self, how=None):
        how = how or (("wave", round(float(self.rng.uniform(0.01, 0.08)), 4), self.i(0, 9)) if self.rng.random() < 0.75 else ("back",))
        self.add("update", how=how, torch=bool(self.i(0, 1)))
        self.accum_dims = None

    def install(self, kind):
        if kind == "set_bvh4":                                              # the model's own words, or the level-0 tree of the current vertices
            self.add(kind, words=self.pick(("model", "level0")))
        else:
            self.add(kind)
        self.accum_dims = None

    # -- observations
    def render(self, mode=None):
        mode = self.i(0, 2) if mode is None else mode
        kw = dict(mode=mode, w=self.i(1, 160), h=self.i(1, 100), cam=self.i(0, 5), stats=self.rng.random() < 0.34, simple=mode != 0 and self.rng.random() < 0.25)
        if mode == 2:
            kw.update(spp=self.i(1, 4), bounces=self.i(0, 6), seed=self.i(1, 99), frame=self.i(0, 20))
        self.add("render", **kw)
        self.accum_dims = None

    def render_shares(self):
        self.add("render_shares", w=self.i(9, 160), h=self.i(9, 100), world=self.i(2, 3), cam=self.i(0, 5), spp=self.i(1, 3), bounces=self.i(0, 4), seed=self.i(1, 99), frame=self.i(0, 9))
        self.accum_dims = None

    def accum_run(self, mid=None):
        w, h = self.i(8, 128), self.i(8, 72)
        if (w, h) == self.accum_dims:
            w += 1
        frames = self.i(2, 5)
        at = self.i(1, frames - 1)
        mid = mid if mid is not None else self.pick(["none", "query", "update"])
        kw = dict(w=w, h=h, frames=frames, first=self.i(0, 20), spp=self.i(1, 3), bounces=self.i(0, 4), seed=self.i(1, 99), cam=self.i(0, 5), mid=mid, at=at)
        if mid == "query":
            kw.update(n=self.pick(N_SMALL), qseed=self.i(1, 999))
        if mid == "update":
            kw.update(how=("wave", round(float(self.rng.uniform(0.01, 0.08)), 4), self.i(0, 9)), torch=bool(self.i(0, 1)))
        self.add("accum_run", **kw)
        self.accum_dims = (w, h)

    def batch_run(self, event=None, targets=None):
        """frames queued under set_batch(k) with no read-back between them, something that arrives while they are pending, more frames, and
        only then the launch that delivers them: every frame goes to a buffer of its own (or all to the context's, where the last one stays)"""
        k = self.i(3, 12)
        event = event or self.pick(BATCH_EVENTS)
        kw = dict(k=k, before=self.i(2, k - 1), event=event, after=self.i(0, 2), targets=targets or self.pick(("buffers", "buffers", "own")),
                  w=self.i(8, 128), h=self.i(8, 72), first=self.i(0, 20), spp=self.i(1, 3), bounces=self.i(0, 4), seed=self.i(1, 99), cam=self.i(0, 5))
        if event == "update":
            kw.update(how=("wave", round(float(self.rng.uniform(0.01, 0.08)), 4), self.i(0, 9)), torch=bool(self.i(0, 1)))
        if event == "query":
            kw.update(n=self.pick(N_SMALL), qseed=self.i(1, 999))
        if event == "set_stream":
            self.stream = "torch" if self.stream == "own" else "own"
            kw.update(to=self.stream)
        self.add("batch_run", **kw)
        self.accum_dims = None

    def views(self):
        order = [int(c) for c in self.rng.permutation(6)[: self.i(5, 6)]]
        order += [self.i(0, 5) for _ in range(self.i(1, 4))]                # and again: hits for the ones still cached, misses for the evicted
        self.add("views", cams=order, w=self.i(40, 120), h=self.i(24, 72), seed=self.i(1, 99))
        self.accum_dims = None

    def large(self, cam="near"):
        self.add("large", cam=cam, frame=self.i(0, 7), seed=self.i(1, 9))
        self.accum_dims = None

    def query(self, family=None, n=None, torch=None, kernel=None):
        family = family or self.pick(FAMILIES)
        n = n if n is not None else (self.pick(N_SMALL) if self.rng.random() < 0.5 else self.i(1000, 5000))
        kw = dict(family=family, n=n, qseed=self.i(1, 999), **self.alternate(family, torch, kernel))
        if family == "nearest_k":
            kw["k"] = self.pick((1, 5, 64))
        if family in ("occlusion", "contains", "signed_distance"):
            kw["samples"] = self.pick((1, 3, 5))
        self.add("query", **kw)

    def refuse(self, which=None):
        self.add("refuse", which=which or self.pick(REFUSALS))
        self.observe_tree()                                                 # the next observation is what it would have been without it

    def observe_tree(self):
        r = self.rng.random()
        if r < 0.3:
            self.add("read_bvh4")
        elif r < 0.5 and self.bvh2:
            self.add("read_bvh2")
        elif r < 0.7:
            self.add("scene_info")
        else:
            self.render()

    def filler(self):
        """one more operation that the state allows, drawn by weight (no query: the chain's batch sizes are laid out on purpose)"""
        table = [("scene_info", 1), ("read_bvh4", 2), ("bvh_cost", 1), ("render", 4), ("render_shares", 1), ("views", 1), ("accum_run", 1), ("batch_run", 2),
                 ("update", 3), ("set_bvh4", 1), ("set_batch", 1), ("flush", 1), ("set_stream", 0.5), ("refuse", 1)]
        if self.bvh2:
            table += [("read_bvh2", 2), ("set_bvh2", 1), ("set_bvh4_wide", 1)]
        names, w = zip(*table)
        k = names[int(self.rng.choice(len(names), p=np.array(w) / sum(w)))]
        if k in ("scene_info", "read_bvh4", "read_bvh2", "bvh_cost", "flush"):
            self.add(k)
        elif k in ("set_bvh2", "set_bvh4", "set_bvh4_wide"):
            self.install(k)
        elif k == "set_batch":
            self.add("set_batch", k=self.i(1, 12))
        elif k == "set_stream":
            self.stream = "torch" if self.stream == "own" else "own"
            self.add("set_stream", to=self.stream)
        else:
            getattr(self, k)()


def scene_count(scene):
    """triangles of a scene record: ("soup", n, seed), ("proc", kind, n), ("deck", layers, seed), ("comb",), ("one",), ("empty",)"""
    return {"empty": lambda: 0, "one": lambda: 1, "deck": lambda: 2 * scene[1], "soup": lambda: scene[1], "proc": lambda: scene[2],
            "comb": lambda: cc.geometry(None, "comb").size // 9}[scene[0]]()


def generate(seed, length=LENGTH):
    """The operation records of session `seed`: the same list for the same arguments.  A session is laid out so that its own coverage
    conditions (coverage()) hold whatever the draws are -- a large scene with the exposure and cover cases, a chain of ever smaller scenes
    with one query family behind each and ever smaller batches within a buffer group, a scene that grows again -- and every size, camera,
    flag, route and filler operation in it is drawn from numpy.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    g = _Gen(rng)
    # 1. a large scene: the exposure mask (taken, voided by an update, taken again, widened for a farther camera), the cover cache, both lazy
    #    BVH2 paths, every way to install a tree, every refusal
    big_n = g.i(30000, 60000)
    g.set_triangles(("proc", g.i(0, 1), big_n))
    g.build()
    g.add("read_bvh2")                                                      # directly behind a build
    g.add("scene_info")
    g.large(); g.large()                                                    # two in a row on one tree version
    g.large("far")                                                          # from farther away than the mask's camera
    g.update(("wave", 0.02, g.i(0, 9)))
    g.large(); g.large()                                                    # behind an update (the mask is stale), and a second
    g.add("read_bvh2")                                                      # behind one update
    g.update(); g.update()                                                  # back to back, nothing between them
    g.add("read_bvh2")                                                      # behind two updates
    g.add("bvh_cost")
    g.views()
    g.accum_run("query"); g.accum_run("update"); g.accum_run("none")
    for mode in rng.permutation(3):
        g.render(int(mode))
    g.render_shares()
    for which in rng.permutation(len(REFUSALS)):
        g.refuse(REFUSALS[int(which)])
    for event in rng.permutation(BATCH_EVENTS):                              # each of them meets pending frames
        g.batch_run(str(event), "buffers")
    g.batch_run(targets="own")
    g.add("set_batch", k=g.i(2, 12)); g.render(2); g.add("flush"); g.update(); g.add("read_bvh4"); g.add("set_batch", k=1)
    g.add("set_stream", to="torch"); g.stream = "torch"
    g.query(n=g.pick(N_SMALL)); g.update(); g.add("read_bvh4"); g.render(2)
    g.add("set_stream", to="own"); g.stream = "own"
    for kind in rng.permutation(["set_bvh2", "set_bvh4", "set_bvh4_wide"]):
        g.install(str(kind)); g.observe_tree()
    g.update(("back",)); g.add("read_bvh4"); g.add("read_bvh2")
    # 2. the largest batch of each buffer group, then ever smaller scenes: behind every smaller set_triangles (and the build it needs) one
    #    family, with a batch smaller than the one before it in its group
    order = {"ray": [str(f) for f in rng.permutation(RAY_FAMILIES)], "list": [str(f) for f in rng.permutation(LIST_FAMILIES)]}
    g.query(order["ray"][-1], 5000, torch=False)                            # (another family than the one that follows it in its group)
    g.query(order["list"][-1], 5000, torch=False)
    sizes = {}
    for grp, fams in order.items():
        k = len(fams)
        large_n = sorted((int(v) for v in rng.choice(np.arange(1000, 5000), k - 4, replace=False)), reverse=True)
        sizes[grp] = large_n + [65, 64, 63, 1]
    chain = [order["ray"].pop(0) if (order["ray"] and (j % 2 == 0 or not order["list"])) else order["list"].pop(0) for j in range(len(FAMILIES))]
    counts = [int(v) for v in np.sort(rng.choice(np.arange(12000, min(big_n, 30000)), 3, replace=False))[::-1]]
    counts += [int(v) for v in np.sort(rng.choice(np.arange(2, 4001), len(FAMILIES) - 4, replace=False))[::-1]] + [1]
    taken = {"ray": 0, "list": 0}
    for j, fam in enumerate(chain):
        n_tris = counts[j]
        g.set_triangles(("proc", g.i(0, 1), n_tris) if n_tris >= 12000 else ("one",) if n_tris == 1 else ("soup", n_tris, g.i(1, 999)))
        g.build()
        grp = GROUP[fam]
        g.query(fam, sizes[grp][taken[grp]], torch=False, kernel=j); taken[grp] += 1        # the host route: the staging buffers keep a stale tail
        if rng.random() < 0.35 and n_tris > 1:
            g.filler()
    g.add("read_bvh4"); g.render(2)
    g.set_triangles(("empty",)); g.build(0); g.add("scene_info"); g.add("read_bvh4"); g.render(1)
    # 3. growing again: one triangle, a deck, a soup -- every buffer smaller than it has been, then larger than its contents again
    g.set_triangles(("one",)); g.build(); g.add("read_bvh2"); g.render(2); g.query("closest_points", 64); g.update(); g.add("read_bvh4")
    g.set_triangles(("deck", g.i(20, 70), g.i(1, 99))); g.build(); g.query("list_hits_sorted"); g.query("list_hits_cap"); g.render(2)
    # the comb of the query case modules with its hand-made chain of a tree (the walks run into the 64-entry stack cap; the twins and the
    # oracle drop what the device drops): installed, never built, so there is no BVH2; only the families with a twin of their own
    g.set_triangles(("comb",)); g.add("set_bvh4", words="comb"); g.add("scene_info"); g.add("read_bvh4"); g.render(2)
    for fam in rng.permutation(["closest_points", "count_hits", "contains", "nearest_k", "radius_search", "list_hits", "box_search"])[:4]:
        g.query(str(fam))
    g.update(); g.add("read_bvh4"); g.render(1); g.add("bvh_cost")
    g.set_triangles(("soup", g.i(1500, 4000), g.i(1, 999))); g.build(); g.add("read_bvh2")
    g.views(); g.render_shares(); g.add("bvh_cost")
    for kind in rng.permutation(["set_bvh2", "set_bvh4", "set_bvh4_wide"]):
        g.install(str(kind)); g.observe_tree()
    g.add("set_batch", k=g.i(2, 12)); g.render(2); g.add("flush"); g.accum_run(); g.add("set_batch", k=1)
    for j, fam in enumerate(rng.permutation(FAMILIES)):                     # every family once more: the torch route, and the next kernel
        g.query(str(fam), torch=True, kernel=chain.index(str(fam)) + 1)
    for which in rng.permutation(len(REFUSALS)):                            # and every refusal
        g.refuse(REFUSALS[int(which)])
    g.batch_run()
    assert len(g.ops) < length, (len(g.ops), length)
    while len(g.ops) < length - 1:
        if rng.random() < 0.4:
            g.query()
        else:
            g.filler()
    g.add("read_bvh4")                                                      # whatever came last is observed
    return g.ops


def line(i, op):
    return "%3d %s" % (i, " ".join([op["op"]] + ["%s=%s" % (k, v) for k, v in op.items() if k != "op"]))


# ---- coverage: conditions on the sequence, decided without a device -------------------------------------------------------------------

def coverage(ops):
    """What the sequence covers, from the records alone (the two exposure conditions need the device: run() adds them)."""
    kinds, families, refusals, met_pending = {}, {}, {}, set()
    for op in ops:
        kinds[op["op"]] = kinds.get(op["op"], 0) + 1
        if op["op"] == "query":
            families.setdefault(op["family"], []).append((op["torch"], op["simple"], op["stats"]))
        if op["op"] == "refuse":
            refusals[op["which"]] = refusals.get(op["which"], 0) + 1
        if op["op"] == "batch_run" and op["before"] >= 2:
            met_pending.add(op["event"])
    n_tris, last_n = 0, {}                          # last_n: group -> (family, n) of its latest query
    behind_larger, behind_smaller_scene = set(), set()
    shrunk, prev_kind, stale2 = False, None, 0
    read2 = set()
    trail = []                                       # state-changing operations since the latest observation
    version_cams, best_cams = set(), 0
    large_after_update, updated, large_run, two_in_a_row, second_after_update, far = False, False, 0, False, False, False
    for op in ops:
        k = op["op"]
        if k == "set_triangles":
            n = scene_count(op["scene"])
            shrunk, n_tris = n < n_tris, n
        if k == "query":
            grp = GROUP[op["family"]]
            prev = last_n.get(grp)
            # only a call that uses the group's own buffers counts: the host route stages in them; the torch route is zero-copy, and of
            # it only the list families still go through d_rd_counts and d_rd_temp
            if prev and prev[0] != op["family"] and prev[1] > op["n"] and (not op["torch"] or grp == "list"):
                behind_larger.add(op["family"])
            last_n[grp] = (op["family"], op["n"])
            since = trail[len(trail) - trail[::-1].index("set_triangles"):] if "set_triangles" in trail else None
            if shrunk and since is not None and all(t == "build_bvh" for t in since):
                behind_smaller_scene.add(op["family"])
        if k == "read_bvh2":
            if prev_kind == "build_bvh":
                read2.add("build")                   # nothing between: the build's own lazy path
            if stale2:
                read2.add("update" if stale2 == 1 else "two updates")
            stale2 = 0
        changes_tree = k == "accum_run" and op["mid"] == "update" or k == "batch_run" and op["event"] in ("update", "set_bvh4")
        if k in ("set_triangles", "build_bvh", "update", "set_bvh2", "set_bvh4", "set_bvh4_wide") or changes_tree:
            version_cams = set(); large_run = 0
        if k == "views":
            version_cams |= set(op["cams"]); best_cams = max(best_cams, len(version_cams))
        if k == "large":
            large_run += 1
            two_in_a_row |= large_run >= 2 and prev_kind == "large"
            second_after_update |= updated and large_run >= 2
            large_after_update |= updated and large_run == 1
            far |= op["cam"] == "far" and large_run >= 2
        if k == "update" or (k == "accum_run" and op["mid"] == "update") or (k == "batch_run" and op["event"] == "update"):
            updated = True
            stale2 += 1                              # updates the BVH2 has not seen yet (the next read_bvh2 refits it)
        if k in ("set_triangles", "build_bvh", "set_bvh2", "set_bvh4", "set_bvh4_wide") or (k == "batch_run" and op["event"] == "set_bvh4"):
            updated = False
        if k in ("set_triangles", "build_bvh", "set_bvh2"):
            stale2 = 0
        if k in STATE_OPS:
            if k != "refuse":
                trail.append(k)
        else:
            trail = []
        prev_kind = k
    return dict(kinds=kinds, families=families, refusals=refusals, met_pending=met_pending, behind_larger=behind_larger, behind_smaller_scene=behind_smaller_scene, read_bvh2=read2, cameras_on_one_version=best_cams,
                large_behind_update=large_after_update, large_second_behind_update=second_after_update, large_two_in_a_row=two_in_a_row, large_far=far)


def check_coverage(cov, device):
    missing = [k for k in STATE_OPS + OBSERVATIONS if cov["kinds"].get(k, 0) < 2]
    assert not missing, "operation kinds that ran less than twice: %s" % missing
    for fam in FAMILIES:                                 # every family at least twice, on both routes and on more than one kernel
        runs = cov["families"].get(fam, [])
        assert len(runs) >= 2 and {r[0] for r in runs} == {False, True}, (fam, runs)
        assert fam == "hit_surfels" or len({r[1:] for r in runs}) >= 2, (fam, runs)
    assert all(cov["refusals"].get(w, 0) >= 2 for w in REFUSALS), cov["refusals"]
    assert cov["met_pending"] == set(BATCH_EVENTS), "never met a pending batch: %s" % sorted(set(BATCH_EVENTS) - cov["met_pending"])
    assert cov["behind_larger"] == set(FAMILIES), "never behind a larger batch of its buffer group: %s" % sorted(set(FAMILIES) - cov["behind_larger"])
    assert cov["behind_smaller_scene"] == set(FAMILIES), "never directly behind a smaller set_triangles: %s" % sorted(set(FAMILIES) - cov["behind_smaller_scene"])
    assert cov["read_bvh2"] == {"build", "update", "two updates"}, cov["read_bvh2"]
    assert cov["cameras_on_one_version"] >= 5, cov["cameras_on_one_version"]
    assert cov["large_two_in_a_row"] and cov["large_behind_update"] and cov["large_second_behind_update"] and cov["large_far"], cov
    if device:
        assert cov["mask_current_before_an_update"] and cov["mask_current_after_an_update"], cov
        assert cov["large_launch_on_a_stale_mask"], cov


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def make_scene(rt, scene):
    kind = scene[0]
    if kind == "soup":
        return random_soup(scene[1], scene[2])
    if kind == "proc":
        return rt.procedural_scene(scene[1], scene[2])
    if kind == "deck":
        return hlc.deck(scene[1], scene[2])[0]
    if kind == "comb":
        return cc.geometry(rt, "comb")
    if kind == "one":
        return np.array([-1, -1, 0, 1, -1, 0, 0, 1, 0], np.float32)
    return np.zeros(0, np.float32)


class Model:
    """Plain data: the triangles and the tree words the context must hold now."""

    def __init__(self, rt, orc):
        self.rt, self.orc = rt, orc
        self.tris = self.base = np.zeros(0, np.float32)
        self.bvh2 = self.bvh4 = None

    @property
    def n(self):
        return self.tris.size // 9

    def set_triangles(self, tris):
        self.tris = self.base = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self.bvh2 = self.bvh4 = None

    def build(self, accel):
        rt, n = self.rt, self.n
        if n == 0:
            self.bvh2, self.bvh4 = np.array([0], np.uint32), np.array([0], np.uint32)
        elif accel == rt.PT_ACCEL_PLOC:
            self.bvh2 = rt.build_bvh2_ploc(self.tris)
            self.bvh4 = rt.collapse_bvh2_to_bvh4_accel(self.bvh2, n, accel)[0]
        else:
            morton, order = rt.morton_sort(self.tris)
            self.bvh2 = self.orc.build_lbvh2(self.tris, morton, order)
            self.bvh4 = rt.collapse_lbvh2_to_bvh4(self.bvh2, n)[0] if accel == 0 else rt.collapse_bvh2_to_bvh4_accel(self.bvh2, n, accel)[0]

    def moved(self, how):
        return self.base.copy() if how[0] == "back" else wave(self.tris, how[1], how[2])

    def update(self, tris):
        self.tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        if self.n:
            self.bvh4 = self.rt.refit_bvh4(self.tris, self.bvh4)
            if self.bvh2 is not None:
                self.bvh2 = self.rt.refit_bvh2(self.tris, self.bvh2)

    def level0(self):
        """(BVH2, BVH4) of build level 0 over the current vertices: Morton sort, the LBVH2 host build, the reference's collapse"""
        morton, order = self.rt.morton_sort(self.tris)
        b2 = self.orc.build_lbvh2(self.tris, morton, order)
        return b2, self.rt.collapse_lbvh2_to_bvh4(b2, self.n)[0]

    def install(self, kind, which="model"):
        """the words the operation hands to the context; the model then holds what the context must (a BVH2 it had stays: set_bvh4 leaves it)"""
        rt = self.rt
        if kind == "set_bvh2":
            words = self.bvh2.copy()
            self.bvh4 = rt.collapse_lbvh2_to_bvh4(words, self.n)[0]
        elif kind == "set_bvh4":
            words = self.bvh4.copy() if which == "model" else cc.comb_tree() if which == "comb" else self.level0()[1]
            self.bvh4 = words.copy()
        else:
            words = rt.bvh2_to_bvh4_wide(self.bvh2)
            self.bvh4 = words.copy()
        return words

    def frame(self, w, h, cam, mode, step=(1, 1), **kw):
        o = self.orc
        p = o.make_params(w, h, self.n, cam[0], cam[1], mode={0: orc_mod.MODE_PACKET, 1: orc_mod.MODE_SINGLE, 2: orc_mod.MODE_PATH}[mode], step=step, **kw)
        img, _, st = o.render(p, self.tris, self.bvh4)
        return img, st


# ---- query inputs (the case modules') and expected results (the twins') ----------------------------------------------------------------

def _take(rec, n):
    """n of the records, spread over the whole set (its quarters are of different kinds)"""
    return np.ascontiguousarray(rec[np.linspace(0, len(rec) - 1, n).astype(np.int64)]) if n < len(rec) else rec


def _aligned(rt, a):
    out = rt._aligned_zeros(a.shape, a.dtype); out[...] = a
    return out


def query_input(rt, tris, op):
    fam, n, s = op["family"], op["n"], op["qseed"]
    m = max(n, 64)
    if fam in ("trace_closest", "trace_any", "hit_surfels"):
        O, D = random_rays(tris, m, s)
        return _aligned(rt, _take(rt.pack_rays(O, D), n))
    if fam in ("count_hits", "list_hits", "list_hits_sorted", "list_hits_cap"):
        rays = cc.ray_set(rt, tris, m, s).copy()
        rays[3::13, 3] = np.resize(np.float32([0.5, 2.0, 0.05, 1.0]), len(rays[3::13]))          # as tests/test_gpu_crossings.py spoils them
        rays[5::17, 3] = 0.0; rays[6::17, 3] = -1.0; rays[7::17, 3] = np.nan; rays[8::17, 3] = -np.inf
        rays[9::17, 0] = np.nan; rays[10::17, 5] = np.nan
        return _aligned(rt, _take(rays, n))
    if fam in ("box_count", "box_search"):
        boxes = bc.box_records(rt, tris, n=m, seed=s).copy()
        boxes[3::29, 0] = np.nan; boxes[4::31, 4] = boxes[4::31, 0] - np.float32(1.0); boxes[6::37, 5] = np.inf
        return _aligned(rt, _take(boxes, n))
    if fam == "contains":
        pts = rt.pack_points(cc.cube_points(m, s))
        pts[11::16, 0] = np.nan
        return _aligned(rt, _take(pts, n))
    if fam == "occlusion":
        sf = cc.surfels_of(clc.query_points(tris, m, s))
        sf[::3, 3] = 0.25; sf[5::37, 3] = 0.0; sf[6::37, 3] = -1.0; sf[7::41, 0] = np.nan; sf[8::41, 3] = np.nan
        return _aligned(rt, _take(sf, n))
    # the point queries: radii drawn (radius_cases.point_records) or +inf, as knn_cases.point_records offers them
    radii = "drawn" if fam.startswith("radius") or s % 2 else "inf"
    pts = kc.point_records(rt, tris, radii, n=m, seed=s).copy()
    pts[1::8, 3] = 0.0; pts[5::16, 0] = np.nan; pts[3::32, 3] = -1.0; pts[7::32, 3] = np.nan      # as tests/knn_torch_cases.py spoils them
    return _aligned(rt, _take(pts, n))


def oracle_hits(orc, tris, bvh4, rays, anyhit):
    """(t, prim, normal) per ray from the oracle's single-ray walk: +inf / MISS / 0 on a miss"""
    n = len(rays)
    t = np.full(n, np.inf, np.float32); prim = np.full(n, MISS, np.uint32); nrm = np.zeros((n, 3), np.float32)
    for i in range(n):
        h, tt, nn, tri = orc.trace_ray(tris, bvh4, rays[i, 0:3], rays[i, 4:7], anyhit=anyhit)
        if h:
            t[i], prim[i], nrm[i] = tt, tri, nn
    return t, prim, nrm


def hit_uv(rt, tris, bvh4, rays, t, prim):
    """u, v of the hits (t, prim) from the hit-list twin over the same rays: the entry of triangle prim in the ray's list, whose t must be
    the oracle's on every bit (0, 0 on a miss)"""
    off, lt, lp, lu, lv = rt.list_hits_bvh4(tris, bvh4, rays)
    u = np.zeros(len(rays), np.float32); v = np.zeros(len(rays), np.float32)
    for i in np.flatnonzero(prim != MISS):
        a, b = int(off[i]), int(off[i + 1])
        k = np.flatnonzero(lp[a:b] == prim[i])
        assert len(k) == 1 and lt[a + k[0]].view(np.uint32) == t[i].view(np.uint32), "the oracle's hit of ray %d is not in the twin's hit list" % i
        u[i], v[i] = lu[a + k[0]], lv[a + k[0]]
    return u, v


def traced_surfels(sf):
    with np.errstate(invalid="ignore"):
        return ~np.isnan(sf[:, 0:7]).any(axis=1) & (sf[:, 3] > 0)


def expected(model, op, rec):
    """(arrays to compare on every word, counters or None, extra arguments of the call) for the query `op` over the records `rec`."""
    rt, tris, b4 = model.rt, model.tris, model.bvh4
    fam, simple, stats = op["family"], op["simple"], op["stats"]
    if fam in ("trace_closest", "trace_any"):
        t, prim, _ = oracle_hits(model.orc, tris, b4, rec, fam == "trace_any")
        u, v = hit_uv(rt, tris, b4, rec, t, prim)
        return [t, prim, u, v], None, {}
    if fam == "hit_surfels":
        t, prim, nrm = oracle_hits(model.orc, tris, b4, rec, False)
        hit = prim != MISS
        O, D = rec[:, 0:3], rec[:, 4:7]
        want = np.zeros((len(rec), 8), np.float32)
        want[:, 0:3], want[:, 4:7] = O, D                                   # a miss: {org, 0, dir, 0}  (tests/test_gpu_occlusion.py::test_hit_surfels)
        P = O + D * np.where(hit, t, np.float32(0))[:, None].astype(np.float32)
        dot = (nrm[:, 0] * D[:, 0] + nrm[:, 1] * D[:, 1]) + nrm[:, 2] * D[:, 2]
        nf = np.where((dot < 0)[:, None], nrm, -nrm)
        want[hit, 0:3], want[hit, 3], want[hit, 4:7] = P[hit], 0.5, nf[hit]
        hits = np.stack([t.view(np.uint32), prim, np.zeros(len(rec), np.uint32), np.zeros(len(rec), np.uint32)], axis=1)
        return [want], None, dict(hits=hits)
    if fam == "closest_points":
        r = rt.closest_points_bvh4(tris, b4, rec, stats=stats, simple=simple)
        return list(r[:4]), (r[4] if stats else None), {}
    if fam == "count_hits":
        r = rt.count_hits_bvh4(tris, b4, rec, stats=stats, simple=simple)
        return [r[0] if stats else r], (r[1] if stats else None), {}
    if fam == "contains":
        kw = dict(samples=op["samples"], seed=op["qseed"], index_base=0xFFFFFF00)
        r = rt.contains_bvh4(tris, b4, rec, stats=stats, simple=simple, **kw)
        return list(r[:3]), (r[3] if stats else None), kw
    if fam == "signed_distance":
        kw = dict(samples=op["samples"], seed=op["qseed"], index_base=7)
        dist, prim, u, v = rt.closest_points_bvh4(tris, b4, rec, simple=simple)
        inside = rt.contains_bvh4(tris, b4, rec, simple=simple, **kw)[0].astype(bool)
        return [np.where(inside, -dist, dist).astype(np.float32), prim, u, v], None, kw
    if fam == "occlusion":
        kw = dict(samples=op["samples"], seed=op["qseed"], bias=1e-4, index_base=3)
        rays = rt.occlusion_rays_host(rec, **kw)
        crossed = rt.count_hits_bvh4(tris, b4, rays) > 0                    # any-hit hits exactly where the count is positive
        tr = traced_surfels(rec)
        unocc = (~crossed).reshape(len(rec), op["samples"]).sum(axis=1).astype(np.uint32)
        unocc[~tr] = 0
        smp = np.where(tr, op["samples"], 0).astype(np.uint32)
        vis = np.where(smp > 0, unocc.astype(np.float32) / np.float32(op["samples"]), np.float32(0)).astype(np.float32)
        return [vis, unocc, smp], None, kw
    if fam == "nearest_k":
        r = rt.nearest_k_bvh4(tris, b4, rec, op["k"], stats=stats, simple=simple)
        return list(r[:4]), (r[4] if stats else None), dict(k=op["k"])
    twin = {"radius": rt.radius_search_bvh4, "list_h": rt.list_hits_bvh4, "box_co": rt.box_search_bvh4, "box_se": rt.box_search_bvh4}[fam[:6]]
    kw = dict(sort=True) if fam == "list_hits_sorted" else {}
    if fam in ("radius_count", "box_count"):
        r = twin(tris, b4, rec, capacity=0, stats=stats, simple=simple)
        return [np.diff(r[0].astype(np.int64)).astype(np.uint32)], (r[-1] if stats else None), {}
    cap = None
    if fam.endswith("_cap"):
        total = int(twin(tris, b4, rec, capacity=0, simple=simple)[0][-1])
        cap = total // 2                                                    # below the total (0 of 0 or 1: offsets only)
        kw["capacity"] = cap
    r = twin(tris, b4, rec, stats=stats, simple=simple, **kw)
    arrays = list(r[:-1] if stats else r)
    return arrays, (r[-1] if stats else None), kw


# ---- the session ----------------------------------------------------------------------------------------------------------------------

def event_counts_launches(event):
    """pt_set_stream ends a timing run, and a query's own launches are not this count's business"""
    return event in ("flush", "update", "set_bvh4", "refuse")


def batch_launches(op):
    """launches of a batch_run: a batch is launched when it is full, when the event arrives (a refused update leaves it queued) and at the end"""
    pending = launches = 0
    for f in range(op["before"] + op["after"]):
        if f == op["before"] and op["event"] != "refuse" and pending:
            launches, pending = launches + 1, 0
        pending += 1
        if pending >= op["k"]:
            launches, pending = launches + 1, 0
    if op["after"] == 0 and op["event"] != "refuse" and pending:
        launches, pending = launches + 1, 0
    return launches + (1 if pending else 0)


class Session:
    def __init__(self, rt, orc, seed, ops, device, torch=None, say=None):
        self.rt, self.orc, self.seed, self.ops, self.device, self.torch = rt, orc, seed, ops, device, torch
        self.model = Model(rt, orc)
        self.ctx = rt.Context(0) if device else None
        self.keep = []                                   # tensors the context may still read
        self.stream = None
        self.step = 0
        self.say = say or (lambda s: None)
        self.updated = False                             # an update since the tree was installed
        self.batch = 1                                   # the batch size the session has set
        self.cov = dict(mask_current_before_an_update=False, mask_current_after_an_update=False, large_launch_on_a_stale_mask=False)

    def close(self):
        if self.ctx is not None:
            self.ctx.close()

    def fail(self, what):
        log = "\n".join(line(i, op) for i, op in enumerate(self.ops[: self.step + 1]))
        head = "session seed %d, step %d: %s" % (self.seed, self.step, what)
        raise SessionMismatch("%s\n%s\nreplay: session_model.run(%d, stop_after=%d)\n%s" % (head, log, self.seed, self.step, head))

    def check(self, ok, what):
        if not ok:
            self.fail(what)

    def np_(self, t):
        """a result of either route as numpy"""
        if self.torch is not None and isinstance(t, self.torch.Tensor):
            if t.dtype == self.torch.uint32:
                return t.view(self.torch.int32).cpu().numpy().view(np.uint32)
            return t.cpu().numpy()
        return t

    def counters(self, want, what):
        if want is not None and self.device:
            st = self.ctx.stats()
            got, exp = {k: st[k] for k in COUNTERS}, {k: want[k] for k in COUNTERS}
            self.check(got == exp, "%s: counters %s, expected %s" % (what, got, exp))

    # -- operations
    def play(self, op):
        getattr(self, "op_" + op["op"])(op)

    def op_set_triangles(self, op):
        tris = make_scene(self.rt, op["scene"])
        self.model.set_triangles(tris)
        if self.device:
            self.ctx.set_triangles(tris)
        self.updated = False

    def op_build_bvh(self, op):
        self.model.build(op["accel"])
        if self.device:
            self.ctx.build_bvh(op["accel"])
        self.updated = False

    def send_update(self, moved, by_torch):
        if not self.device:
            return
        if by_torch:
            t = self.torch.from_numpy(moved).cuda()
            self.keep.append(t)
            self.ctx.update_triangles(t)
        else:
            self.ctx.update_triangles(moved)

    def op_update(self, op):
        moved = self.model.moved(op["how"])
        self.model.update(moved)
        self.send_update(moved, op["torch"])
        self.updated = True

    def install(self, kind, which="model"):
        words = self.model.install(kind, which)
        if self.device:
            (self.ctx.set_bvh2 if kind == "set_bvh2" else self.ctx.set_bvh4)(words)
        self.updated = False

    def op_set_bvh2(self, op):
        self.install("set_bvh2")

    def op_set_bvh4(self, op):
        self.install("set_bvh4", op["words"])

    def op_set_bvh4_wide(self, op):
        self.install("set_bvh4_wide")

    def op_set_batch(self, op):
        self.batch = op["k"]
        if self.device:
            self.ctx.set_batch(op["k"])

    def op_flush(self, op):
        if self.device:
            self.ctx.flush()

    def op_set_stream(self, op):
        if not self.device:
            return
        if op["to"] == "torch":
            self.stream = self.torch.cuda.Stream()
            self.ctx.set_stream(self.stream.cuda_stream)
        else:
            self.ctx.synchronize()
            self.ctx.set_stream(None)

    def op_refuse(self, op):
        if not self.device:
            return
        rt, ctx, m = self.rt, self.ctx, self.model
        which = op["which"]
        if which == "update_count":
            call, code, text = (lambda: ctx.update_triangles(np.zeros(9 * (m.n + 1), np.float32))), 1, "pt_update_triangles: an update keeps the triangle count (pt_set_triangles changes it)"
        elif which == "build_accel_7":
            call, code, text = (lambda: ctx.build_bvh(7)), 1, "pt_build_bvh_accel: accel must be 0 (reference), 1 (area collapse) or 2 (PLOC)"
        elif which == "query_2_32":
            rays = rt.pack_rays(np.zeros((4, 3)), np.ones((4, 3))); hits = rt._aligned_zeros((4, 4), np.uint32)
            call = lambda: ctx._ck(rt.lib.pt_trace_rays_host(ctx.h, rays.ctypes.data_as(C.POINTER(rt.PtRay)), C.c_uint64(1 << 32), C.c_uint32(0), hits.ctypes.data_as(C.POINTER(rt.PtHit))))
            code, text = 1, "pt_trace_rays_host: more than 2^32 - 1 rays"
        else:
            short = np.zeros(rt.compute_bvh2_sizing(m.n)["bytes"] // 4 - 5, np.uint32); short[0] = rt.compute_bvh2_sizing(m.n)["numNodes2"]
            call, code, text = (lambda: ctx.set_bvh2(short)), 5, "pt_set_bvh2: buffer does not match 2N-1 nodes of the uploaded triangles"
        try:
            call()
        except rt.PtError as e:
            self.check(e.code == code and str(e) == "libmi355pt error %d: %s" % (code, text), "refusal %s answered %r" % (which, str(e)))
            return
        self.fail("%s was accepted" % which)

    def op_scene_info(self, op):
        m = self.model
        want = {"numTris": m.n, "numNodes2": int(m.bvh2[0]) if m.bvh2 is not None else 0, "numNodes4": int(m.bvh4[0])}
        if self.device:
            got = self.ctx.scene_info()
            self.check(got == want, "scene_info %s, expected %s" % (got, want))

    def op_read_bvh4(self, op):
        if self.device:
            got = self.ctx.read_bvh4()
            want = self.model.bvh4
            self.check(same(got, want), "read_bvh4: %d words, expected %d" % (got.size, want.size) if got.shape != want.shape else
                       "read_bvh4 differs from the model's words at %s" % np.flatnonzero(got != want)[:8])

    def op_read_bvh2(self, op):
        if self.device:
            got = self.ctx.read_bvh2()
            self.check(same(got, self.model.bvh2), "read_bvh2 differs from the model's words")

    def op_bvh_cost(self, op):
        want = self.rt.bvh4_cost(self.model.bvh4)
        if self.device:
            got = self.ctx.bvh_cost()
            self.check(abs(got - want) <= int(self.model.bvh4[0]) * 2.0 ** -51 * want, "bvh_cost %r, expected %r" % (got, want))

    def frame_kw(self, op):
        return dict(spp=op["spp"], max_bounces=op["bounces"], seed=op["seed"], frame=op["frame"]) if op["mode"] == 2 else {}

    def op_render(self, op):
        rt, m = self.rt, self.model
        cam = CAMS[op["cam"]]
        kw = self.frame_kw(op)
        ref, ost = m.frame(op["w"], op["h"], cam, op["mode"], **kw)
        if self.device:
            self.ctx.render(self.ctx.make_params(op["w"], op["h"], cam[0], cam[1], mode=op["mode"], stats=op["stats"], simple_kernel=op["simple"], **kw))
            self.check(same(self.ctx.read_radiance(), ref), "the frame differs from the oracle's")
            self.counters(ost if op["stats"] else None, "render")

    def op_render_shares(self, op):
        rt, m = self.rt, self.model
        cam = CAMS[op["cam"]]
        w, h, world = op["w"], op["h"], op["world"]
        kw = dict(spp=op["spp"], max_bounces=op["bounces"], seed=op["seed"], frame=op["frame"])
        ref, _ = m.frame(w, h, cam, 2, **kw)
        if self.device:
            ctx, torch = self.ctx, self.torch
            stride = max(rt.tile_layout(w, h, r, world)[1] for r in range(world))
            g = torch.zeros(world * stride, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for r in range(world):
                ctx.set_compact_buffer(g.data_ptr() + r * stride * 4, stride)
                ctx.render(ctx.make_params(w, h, cam[0], cam[1], mode=rt.PT_MODE_PATH, tile_rank=r, tile_count=world, **kw))
            ctx.synchronize()
            ctx.deinterleave(g.data_ptr(), stride, w, h, world)
            img = ctx.read_radiance(w, h)
            ctx.set_compact_buffer(0, 0)
            self.check(same(img, ref), "the frame put together from %d tile shares differs from the oracle's" % world)

    def op_accum_run(self, op):
        rt, m = self.rt, self.model
        cam = CAMS[op["cam"]]
        w, h, first, start = op["w"], op["h"], op["first"], 0
        kw = dict(spp=op["spp"], max_bounces=op["bounces"], seed=op["seed"])
        for f in range(op["frames"]):
            if f == op["at"] and op["mid"] == "query":
                self.op_query(dict(op="query", family="closest_points", n=op["n"], qseed=op["qseed"], torch=False, simple=False, stats=False))
            if f == op["at"] and op["mid"] == "update":
                moved = m.moved(op["how"])
                m.update(moved)
                self.send_update(moved, op["torch"])
                self.updated = True
                start = f                                                   # the run starts again (tests/test_gpu_refit.py::test_accumulation_restarts_after_an_update)
            if self.device:
                self.ctx.render(self.ctx.make_params(w, h, cam[0], cam[1], mode=rt.PT_MODE_PATH, frame=first + f, accumulate=True, **kw))
        ref, _ = m.frame(w, h, cam, 2, frame=first + start, accum_frames=op["frames"] - start, **kw)
        if self.device:
            self.check(self.ctx.accum_info().samples == (op["frames"] - start) * op["spp"], "accumulated samples %d" % self.ctx.accum_info().samples)
            self.check(same(self.ctx.read_radiance(), ref), "the accumulated frame differs from the oracle's")

    def op_batch_run(self, op):
        """op["before"] frames queued under set_batch(k) and not launched (before < k, nothing reads back), the event, op["after"] more frames,
        then the launch: each frame must be the oracle's for the geometry and the tree that were current when it was submitted."""
        rt, m = self.rt, self.model
        cam = CAMS[op["cam"]]
        w, h, total = op["w"], op["h"], op["before"] + op["after"]
        kw = dict(spp=op["spp"], max_bounces=op["bounces"], seed=op["seed"])
        own = op["targets"] == "own"
        bufs = []
        if self.device:
            self.ctx.set_batch(op["k"])
            if not own:
                bufs = [self.torch.zeros((h, w, 4), dtype=self.torch.float32, device="cuda") for _ in range(total)]
                self.torch.cuda.synchronize()
        refs = []
        # the launches pt_render records while timing is on say that the frames were pending when the event arrived: one launch per full
        # batch, one for what the event (all but the refused call) or the end finds queued -- fewer launches than frames
        counted = self.device and event_counts_launches(op["event"])
        if counted:
            self.ctx.timing_begin(total + 2)

        def submit(f):
            refs.append(m.frame(w, h, cam, 2, frame=op["first"] + f, **kw)[0])
            if self.device:
                if not own:
                    self.ctx.set_output_buffer(bufs[f].data_ptr(), w * h * 4)
                self.ctx.render(self.ctx.make_params(w, h, cam[0], cam[1], mode=rt.PT_MODE_PATH, frame=op["first"] + f, **kw))
        for f in range(op["before"]):
            submit(f)
        event = op["event"]
        if event == "flush":
            self.op_flush(op)
        elif event == "update":
            self.op_update(op)
        elif event == "set_bvh4":
            self.install("set_bvh4", "level0")
        elif event == "set_stream":
            self.op_set_stream(op)
        elif event == "query":
            self.op_query(dict(op="query", family="closest_points", n=op["n"], qseed=op["qseed"], torch=False, simple=False, stats=False))
        else:
            self.op_refuse(dict(which="update_count"))                      # refused before anything is launched: the frames stay queued
        for f in range(op["before"], total):
            submit(f)
        if not self.device:
            return
        if own:
            self.check(same(self.ctx.read_radiance(), refs[-1]), "the last of %d queued frames differs from the oracle's" % total)
        else:
            self.ctx.set_output_buffer(0, 0)                                # launches what is queued and waits
            for f in range(total):
                self.check(same(bufs[f].cpu().numpy(), refs[f]), "queued frame %d of %d (%d before the %s) differs from the oracle's" % (f, total, op["before"], event))
        if counted:
            launches = len(self.ctx.timing_collect(total + 2))
            self.check(launches == batch_launches(op), "%d launches for %d frames, expected %d" % (launches, total, batch_launches(op)))
        self.ctx.set_batch(self.batch)

    def op_views(self, op):
        rt, m = self.rt, self.model
        frames = {}
        for c in op["cams"]:
            cam = CAMS[c]
            if c not in frames:
                frames[c] = m.frame(op["w"], op["h"], cam, 2, spp=2, max_bounces=2, seed=op["seed"])[0]
            if self.device:
                self.ctx.render(self.ctx.make_params(op["w"], op["h"], cam[0], cam[1], mode=rt.PT_MODE_PATH, spp=2, max_bounces=2, seed=op["seed"]))
                self.check(same(self.ctx.read_radiance(), frames[c]), "the view from camera %d differs from the oracle's" % c)

    def op_large(self, op):
        rt, m = self.rt, self.model
        pos = LARGE_CAMS[op["cam"]]
        w, h = LARGE["w"], LARGE["h"]
        kw = dict(spp=LARGE["spp"], max_bounces=LARGE["bounces"], seed=op["seed"], frame=op["frame"])
        ref, _ = m.frame(w, h, (pos, (0, 0, 0, 1)), 2, step=(16, 16), **kw)
        if not self.device:
            return
        ctx = self.ctx
        before = ctx.debug_exposure(None, want_mask=False)["valid"]
        ctx.render(ctx.make_params(w, h, pos, mode=rt.PT_MODE_PATH, **kw))
        img = ctx.read_radiance()
        after = ctx.debug_exposure(None, want_mask=False)["valid"]
        self.check(same(img[::16, ::16], ref[::16, ::16]), "the large launch differs from the oracle on the 16 x 16 subgrid (mask current before: %s, after: %s)" % (before, after))
        if before or after:
            self.cov["mask_current_after_an_update" if self.updated else "mask_current_before_an_update"] = True
        if self.updated and not before:
            self.cov["large_launch_on_a_stale_mask"] = True
        # a second, new context with the model's triangles and words and nothing else: no mask, no cover
        other = rt.Context(0)
        try:
            other.set_triangles(m.tris); other.set_bvh4(m.bvh4)
            other.render(other.make_params(w, h, pos, mode=rt.PT_MODE_PATH, **kw))
            self.check(same(img, other.read_radiance()), "the large launch differs from a new context's frame (mask current before: %s, after: %s)" % (before, after))
        finally:
            other.close()

    def op_query(self, op):
        rt, m = self.rt, self.model
        fam = op["family"]
        rec = query_input(rt, m.tris, op)
        want, want_st, kw = expected(m, op, rec)
        if not self.device:
            return
        ctx = self.ctx
        arg = rec
        if op["torch"]:
            arg = self.torch.from_numpy(rec).cuda()
            self.keep.append(arg)
        flags = dict(simple=op["simple"], stats=op["stats"])
        if fam in ("trace_closest", "trace_any"):
            got = ctx.trace_rays(arg, any_hit=fam == "trace_any", **flags)
        elif fam == "hit_surfels":
            hits = kw["hits"]
            if op["torch"]:
                hits = self.torch.from_numpy(hits.view(np.int32)).cuda(); self.keep.append(hits)
            got = [self.np_(ctx.hit_surfels(arg, hits, 0.5))]
        elif fam == "closest_points":
            got = ctx.closest_points(arg, **flags)
        elif fam == "count_hits":
            got = [ctx.count_hits(arg, **flags)]
        elif fam == "contains":
            got = ctx.contains(arg, **flags, **kw)
        elif fam == "signed_distance":
            got = ctx.signed_distance(arg, simple=op["simple"], **kw)
        elif fam == "occlusion":
            got = ctx.occlusion(arg, **flags, **kw)
        elif fam == "nearest_k":
            got = ctx.nearest_k(arg, op["k"], **flags)
        elif fam == "radius_count":
            got = [ctx.radius_count(arg, **flags)]
        elif fam == "box_count":
            got = [ctx.box_count(arg, **flags)]
        elif fam.startswith("radius_search"):
            got = ctx.radius_search(arg, **flags, **kw)
        elif fam.startswith("list_hits"):
            got = ctx.list_hits(arg, **flags, **kw)
        else:
            got = ctx.box_search(arg, **flags, **kw)
        got = [self.np_(x) for x in got]
        if op["torch"] and "capacity" in kw:             # the torch route with a capacity hands out `capacity` entries: those from the total on are not written
            self.check(all(len(x) == kw["capacity"] for x in got[1:]), "%s: %d entries handed out for capacity %d" % (fam, len(got[1]), kw["capacity"]))
            got = [got[0]] + [x[: len(want[1])] for x in got[1:]]
        self.check(len(got) == len(want), "%s: %d arrays, expected %d" % (fam, len(got), len(want)))
        for k, (a, b) in enumerate(zip(got, want)):
            if not same(a, b):
                a2, b2 = bits(a), bits(b)
                where = np.flatnonzero((a2 != b2).reshape(len(a2), -1).any(axis=1))[:8] if a2.shape == b2.shape else "shapes %s, %s" % (a2.shape, b2.shape)
                self.fail("%s: result array %d differs from the twin's at %s" % (fam, k, where))
        self.counters(want_st, fam)


def run(seed, length=LENGTH, stop_after=None, device=True, ops=None, rt=None, orc=None, say=None):
    """Plays session `seed` (or the records `ops`) and checks every observation where it happens; stop_after=k replays the prefix up to and
    including step k.  device=False: the model alone, twins and oracle, no context.  Returns the coverage, with the operation count and
    the wall time."""
    import importlib
    rt = rt or importlib.import_module("raytracer-public_amd")
    orc = orc or orc_mod.load()
    torch_mod = sys.modules.get("torch") if device else None
    if device:
        assert rt._TORCH_FIRST and torch_mod is not None, "the device leg needs `import torch` before the package (the torch routes)"
    ops = generate(seed, length) if ops is None else ops
    if stop_after is not None:
        ops = ops[: stop_after + 1]
    s = Session(rt, orc, seed, ops, device, torch_mod, say)
    t0 = time.time()
    try:
        for i, op in enumerate(ops):
            s.step = i
            t1 = time.time()
            try:
                s.play(op)
            except SessionMismatch:
                raise
            except Exception as e:                        # an error of the library or of a reference: the same message, with the log
                s.fail("%s: %s" % (type(e).__name__, e))
            s.say("%s  [%.3f s]" % (line(i, op), time.time() - t1))
        if device:
            s.ctx.synchronize()
    finally:
        s.close()
    cov = coverage(ops)
    cov.update(s.cov)
    cov.update(operations=len(ops), seconds=time.time() - t0)
    return cov


if __name__ == "__main__":
    leg, seed = sys.argv[1], int(sys.argv[2])
    stop = int(sys.argv[3]) if len(sys.argv) > 3 else None
    cov = run(seed, stop_after=stop, device=leg == "gpu", say=(print if os.environ.get("SESSION_LOG") else None))
    if stop is None:
        check_coverage(cov, leg == "gpu")
    print("ok session %d: %d operations in %.1f s" % (seed, cov["operations"], cov["seconds"]))
