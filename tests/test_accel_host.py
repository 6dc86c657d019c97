"""Opt-in tree quality (include/mi355pt.h PT_ACCEL_*), host side: the area-guided collapse and the PLOC BVH2
host twins.  Structural invariants of what they emit (restated from tests/test_bvh_invariants.py), the PLOC BVH2's layout against
the oracle's LBVH2 leaves, and the tree quality the option exists for, pinned by the CPU oracle's node counts and images."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import orc as orc_mod
from scenes import pack_box

LEAF = 0x80000000
INVALID = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bvh4_wide_ref")
SCENE_SEED = 20260109


def half(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def unpack_bounds(w):
    w = np.asarray(w, np.uint32)
    return (np.stack([half(w[..., 0] & 0xFFFF), half(w[..., 0] >> 16), half(w[..., 1] & 0xFFFF)], -1),
            np.stack([half(w[..., 1] >> 16), half(w[..., 2] & 0xFFFF), half(w[..., 2] >> 16)], -1))


def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3), dtype=np.float32) * 2 - 1
    return (c + (rng.random((n, 3, 3), dtype=np.float32) - 0.5) * 0.2).astype(np.float32).reshape(-1)


def degenerate(kind):
    """The inputs of tests/test_gpu_parity.py::test_build_bvh_degenerate_inputs."""
    rng = np.random.default_rng(3)
    if kind == "identical":
        return np.tile(np.array([0.1, 0.2, 0.3, 0.4, 0.2, 0.3, 0.1, 0.5, 0.3], np.float32), 300)
    if kind == "coplanar":
        tris = rng.uniform(-1, 1, (500, 3, 3)).astype(np.float32); tris[:, :, 2] = 0.25
        return tris.reshape(-1)
    if kind == "two_clusters":
        a = rng.uniform(-1e-3, 1e-3, (200, 3, 3)).astype(np.float32) + np.float32(-0.9)
        b = rng.uniform(-1e-3, 1e-3, (200, 3, 3)).astype(np.float32) + np.float32(0.9)
        return np.concatenate([a, b]).reshape(-1)
    if kind == "tiny":
        return rng.uniform(-3e-6, 3e-6, (400, 3, 3)).astype(np.float32).reshape(-1)
    if kind == "mixed_zero":
        tris = rng.uniform(-1, 1, (600, 3, 3)).astype(np.float32)
        zeros = np.array([0.0, -0.0, 1e-9, -1e-9, 4e-9, -4e-9], np.float32)
        for axis in range(3):
            pick = rng.random((600, 3)) < 0.5
            tris[:, :, axis][pick] = zeros[rng.integers(0, 6, int(pick.sum()))]
        return tris.reshape(-1)
    tris = rng.uniform(-1, 1, (256, 3, 3)).astype(np.float32)
    tris[::3, :, 0] = np.float32(-0.0); tris[1::3, :, 1] = np.float32(0.0)
    return tris.reshape(-1)


DEGENERATE = ["identical", "coplanar", "two_clusters", "tiny", "signed_zero", "mixed_zero"]


def assert_bvh4_invariants(b4, n4, n):
    """Pre-order, one leaf per triangle, 2..4 children packed to the front, every box contains its children."""
    assert b4[0] == n4 and len(b4) == 1 + 8 * n4 and n <= n4 <= 2 * n - 1
    rec = b4[1:].reshape(n4, 8)
    leaf = (rec[:, 7] & LEAF) != 0
    assert leaf.sum() == n and np.array_equal(np.sort(rec[leaf, 7] & 0x7FFFFFFF), np.arange(n, dtype=np.uint32))
    assert np.all(rec[leaf, 3:7] == INVALID) and np.all(rec[~leaf, 7] == 0)
    kids = rec[:, 3:7]
    valid = kids != INVALID
    cnt = valid.sum(1)
    assert np.all(cnt[~leaf] >= 2) and np.all(cnt[~leaf] <= 4)
    assert np.all(valid[:, :-1] >= valid[:, 1:])
    internal = np.nonzero(~leaf)[0]
    assert np.array_equal(kids[internal, 0], internal.astype(np.uint32) + 1)
    all_kids = kids[valid]
    assert len(np.unique(all_kids)) == len(all_kids) == n4 - 1 and 0 not in all_kids
    par = np.repeat(np.arange(n4), 4).reshape(n4, 4)[valid]
    assert np.all(all_kids > par)
    # pre-order: subtrees are contiguous id ranges -- each child starts where its previous sibling's subtree ended
    size = np.ones(n4, np.int64)
    for i in internal[::-1]:
        size[i] = 1 + size[kids[i][valid[i]]].sum()
    for i in internal:
        k = kids[i][valid[i]].astype(np.int64)
        assert np.array_equal(k, i + 1 + np.concatenate([[0], np.cumsum(size[k])[:-1]]))
    # every box contains its children's -- except where the reference's f16 re-encode (PathTracer.js:42-51) flushes a child bound
    # below the f16 normal range (|x| < 2^-14) to zero, which every collapse level reproduces
    mn, mx = unpack_bounds(rec[:, :3])
    tiny = np.float32(2.0 ** -14)
    for s in range(4):
        sel = valid[:, s]
        c = kids[sel, s]
        assert np.all((mn[sel] <= mn[c]) | ((np.abs(mn[c]) < tiny) & (mn[sel] == 0)))
        assert np.all((mx[sel] >= mx[c]) | ((np.abs(mx[c]) < tiny) & (mx[sel] == 0)))


def assert_ploc_bvh2(rt, orc, tris, b2):
    n = tris.size // 9
    nn2 = 2 * n - 1
    assert b2.dtype == np.uint32 and len(b2) == 1 + 6 * nn2 and b2[0] == nn2
    lb = orc.build_lbvh2(tris)
    # leaves N-1+k: exactly the LBVH's leaf words (Morton-sorted triangle k)
    assert np.array_equal(b2[1 + 6 * (n - 1):], lb[1 + 6 * (n - 1):])
    if n == 1:
        return
    rec = b2[1:].reshape(nn2, 6)
    inner = rec[: n - 1]
    assert np.all(inner[:, 5] == 0)
    kids = inner[:, 3:5].reshape(-1)
    # root 0; every other node has exactly one parent, and that parent's index is smaller
    assert len(np.unique(kids)) == len(kids) == nn2 - 1 and 0 not in kids and np.all(kids < nn2)
    par = np.repeat(np.arange(n - 1), 2)
    assert np.all(kids > par)
    # internal bounds: the children's union (-0 below +0), then one f16 step outwards (BVHBuilder.wgsl:63-102, 242-275) -- in the
    # order-preserving integer form of f16, a step is +-1
    h = np.stack([rec[:, 0] & 0xFFFF, rec[:, 0] >> 16, rec[:, 1] & 0xFFFF, rec[:, 1] >> 16, rec[:, 2] & 0xFFFF, rec[:, 2] >> 16], -1).astype(np.int64)
    o = ord16(h)
    l, r = inner[:, 3].astype(np.int64), inner[:, 4].astype(np.int64)
    want = np.concatenate([np.minimum(o[l, :3], o[r, :3]) - 1, np.maximum(o[l, 3:], o[r, 3:]) + 1], -1)
    assert np.array_equal(o[: n - 1], want)
    mn, mx = unpack_bounds(rec[:, :3])
    assert np.all(mn[: n - 1] <= np.minimum(mn[l], mn[r])) and np.all(mx[: n - 1] >= np.maximum(mx[l], mx[r]))


def ord16(bits):
    """f16 bits -> an integer that orders like the value (-0 just below +0)."""
    return np.where(bits & 0x8000, (~bits) & 0xFFFF, bits ^ 0x8000)


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (3, 2), (50, 3), (4097, 4), (30000, 5)])
def test_ploc_bvh2_and_area_collapses_on_soups(rt, orc, n, seed):
    tris = soup(n, seed)
    b2 = rt.build_bvh2_ploc(tris)
    assert_ploc_bvh2(rt, orc, tris, b2)
    for accel in (rt.PT_ACCEL_AREA_COLLAPSE, rt.PT_ACCEL_PLOC):
        b4, n4 = rt.collapse_bvh2_to_bvh4_accel(b2, n, accel)
        assert_bvh4_invariants(b4, n4, n)
    lb = orc.build_lbvh2(tris)
    b4, n4 = rt.collapse_bvh2_to_bvh4_accel(lb, n, rt.PT_ACCEL_AREA_COLLAPSE)
    assert_bvh4_invariants(b4, n4, n)
    # accel 0 is the reference collapse, word for word
    b40, _ = rt.collapse_bvh2_to_bvh4_accel(lb, n, rt.PT_ACCEL_REFERENCE)
    assert np.array_equal(b40, orc.collapse_bvh4(lb, n)[0])
    assert np.array_equal(b40, rt.collapse_lbvh2_to_bvh4(lb, n)[0])


@pytest.mark.parametrize("kind", DEGENERATE)
def test_ploc_and_area_collapse_on_degenerate_inputs(rt, orc, kind):
    tris = degenerate(kind)
    n = tris.size // 9
    b2 = rt.build_bvh2_ploc(tris)
    assert_ploc_bvh2(rt, orc, tris, b2)
    assert np.array_equal(rt.build_bvh2_ploc(tris), b2)                 # deterministic
    for bvh2 in (b2, orc.build_lbvh2(tris)):
        b4, n4 = rt.collapse_bvh2_to_bvh4_accel(bvh2, n, rt.PT_ACCEL_PLOC)
        assert_bvh4_invariants(b4, n4, n)


@pytest.mark.parametrize("kind", [0, 1])
def test_procedural_scenes_keep_the_invariants(rt, orc, kind):
    tris = rt.procedural_scene(kind, 20000)
    b2 = rt.build_bvh2_ploc(tris)
    assert_ploc_bvh2(rt, orc, tris, b2)
    b4, n4 = rt.collapse_bvh2_to_bvh4_accel(b2, 20000, rt.PT_ACCEL_PLOC)
    assert_bvh4_invariants(b4, n4, 20000)


def test_invalid_accel_is_rejected(rt):
    tris = soup(10, 0)
    b2 = rt.build_bvh2_ploc(tris)
    with pytest.raises(rt.PtError):
        rt.collapse_bvh2_to_bvh4_accel(b2, 10, 3)
    b4, n4 = rt.collapse_bvh2_to_bvh4_accel(b2, 10, rt.PT_ACCEL_PLOC)          # the library is still usable
    assert_bvh4_invariants(b4, n4, 10)


def test_area_collapse_expands_the_largest_internal_entry(rt):
    """A hand-made BVH2 where the first internal entry is the smaller one: the reference expands it, the area rule the other one."""
    box = pack_box
    # 5 leaves; root 0 = (1, 2); node 1 = (5, 6) small; node 2 = (3, 7) large; node 3 = (4, 8) large
    n = 5
    b2 = np.zeros(1 + 6 * 9, np.uint32)
    b2[0] = 9
    recs = {0: (box((0, 0, 0), (8, 8, 8)), 1, 2), 1: (box((0, 0, 0), (1, 1, 1)), 5, 6), 2: (box((0, 0, 0), (8, 8, 8)), 3, 7),
            3: (box((4, 4, 4), (8, 8, 8)), 4, 8)}
    for i, (w, l, r) in recs.items():
        b2[1 + 6 * i: 1 + 6 * i + 6] = [w[0], w[1], w[2], l, r, 0]
    for k in range(5):
        w = box((k, k, k), (k + 0.5, k + 0.5, k + 0.5))
        b2[1 + 6 * (4 + k): 1 + 6 * (5 + k)] = [w[0], w[1], w[2], 0, 0, LEAF | k]
    ref, _ = rt.collapse_bvh2_to_bvh4_accel(b2, n, rt.PT_ACCEL_REFERENCE)
    area, _ = rt.collapse_bvh2_to_bvh4_accel(b2, n, rt.PT_ACCEL_AREA_COLLAPSE)
    root_ref, root_area = ref[1:9], area[1:9]
    # reference: root's entries (1, 2) -> expand 1 (first internal) -> (5, 6, 2) -> expand 2 -> (5, 6, 3, 7)
    # area:      root's entries (1, 2) -> expand 2 (larger)         -> (1, 3, 7) -> expand 3 (area 48 > 3) -> (1, 4, 8, 7)
    def leaf_of(b4, c):
        return int(b4[1 + 8 * c + 7])
    assert (leaf_of(ref, root_ref[3]) & LEAF) and (leaf_of(ref, root_ref[4]) & LEAF)         # slots 0, 1 are leaves 5, 6 (triangles 1, 2)
    assert [leaf_of(ref, c) & 0xFF for c in root_ref[3:5]] == [1, 2]
    kinds = [leaf_of(area, c) for c in root_area[3:7]]
    assert kinds[0] == 0                                              # slot 0: internal node 1, not expanded
    assert [k & 0xFF for k in kinds[1:]] == [0, 4, 3] and all(k & LEAF for k in kinds[1:])


def _grid_counts(orc, tris, bvh4, cam, quat):
    n = tris.size // 9
    p = orc.make_params(1920, 1080, n, cam, quat, mode=orc_mod.MODE_PATH, spp=4, max_bounces=8, seed=1, step=(16, 16))
    img, st = orc.render_mt(p, tris, bvh4)
    return img[::16, ::16], st["nodes_examined"] / (st["rays_closest"] + st["rays_shadow"]), st


@pytest.mark.parametrize("config", ["C4", "C2"])
def test_tree_quality_on_the_procedural_configurations(rt, orc, config):
    """Nodes per traced ray on the every-16th-pixel grid (4 spp, 8 bounces): the reason the option exists.  Measured
    C4 120.4 -> 104.1 (accel 1) -> 77.9 (accel 2), C2 37.9 -> 32.2 / 32.2; pinned with margins.  The images are the same picture
    (only exact-t ties may pick another triangle)."""
    if config == "C4":
        tris = rt.procedural_scene(rt.SCENE_SPONZA_CLASS, 262144, SCENE_SEED)
        cam, quat, limits = (0.55, -0.05, 0.05), (0.0, 0.6630, 0.0, 0.7486), {1: 0.92, 2: 0.75}
    else:
        tris = rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 871414, SCENE_SEED)
        cam, quat, limits = (0, 0, 2.5), (0, 0, 0, 1), {1: 0.92, 2: 0.92}
    n = tris.size // 9
    lb = orc.build_lbvh2(tris)
    b0, _ = orc.collapse_bvh4(lb, n)
    img0, npr0, st0 = _grid_counts(orc, tris, b0, cam, quat)
    trees = {1: rt.collapse_bvh2_to_bvh4_accel(lb, n, 1)[0], 2: rt.collapse_bvh2_to_bvh4_accel(rt.build_bvh2_ploc(tris), n, 2)[0]}
    for accel, b4 in trees.items():
        img, npr, st = _grid_counts(orc, tris, b4, cam, quat)
        diff = int(np.any(img != img0, axis=-1).sum())
        rel = float(np.linalg.norm(img - img0) / np.linalg.norm(img0))
        print("%s accel %d: nodes/ray %.2f vs %.2f (%.3f), nodes4 %d vs %d, max stack %d vs %d, differing pixels %d, rel L2 %.3g"
              % (config, accel, npr, npr0, npr / npr0, b4[0], b0[0], st["max_stack"], st0["max_stack"], diff, rel))
        assert npr <= limits[accel] * npr0, (accel, npr, npr0)
        assert rel <= 1e-4
        assert st["stack_drops"] == 0
        assert b4[0] <= 1.05 * b0[0]


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/bvh4_wide_ref was not built (reference checkout absent)")
def test_reference_converter_accepts_the_ploc_bvh2(rt):
    """The reference's own BVH2 -> BVH4_wide tool reads a PLOC BVH2 (a data/BVH2.bin of level 2) like any other."""
    for n, seed in ((1, 0), (37, 1), (1000, 2)):
        tris = soup(n, seed)
        b2 = rt.build_bvh2_ploc(tris)
        with tempfile.TemporaryDirectory() as d:
            a, b = os.path.join(d, "BVH2.bin"), os.path.join(d, "BVH4_wide.bin")
            b2.tofile(a)
            subprocess.check_call([REF_BIN, a, b], stdout=subprocess.DEVNULL)
            assert np.array_equal(np.fromfile(b, np.uint32), rt.bvh2_to_bvh4_wide(b2))


def test_build_kernels_use_no_scratch():
    """Compile-only: the area-guided collapse and the PLOC kernels keep everything in registers and LDS.  (The reference-rule
    instantiation, collapse_expand_kernel<false>, is the level-0 kernel as it was, dynamically indexed child array and all.)"""
    import re
    csrc = os.path.join(ROOT, "raytracer-public_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "resource-usage-build"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = b.split()[0]
        if "ploc_" in name or "collapse_expand_kernelILb1E" in name:
            seen[name] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    assert len(seen) == 5, sorted(seen)
    assert all(v == 0 for v in seen.values()), seen
