"""Shared by the refit tests (tests/test_refit_host.py, tests/test_gpu_refit.py, tests/refit_torch_cases.py): the `--animate`
displacement of the Node driver restated in numpy float32 (tools/README.md), the refit rules of include/mi355pt.h restated in numpy,
the tree-quality sum in f64, and the trees of the three build levels."""
import numpy as np

LEAF = 0x80000000
INVALID = 0xFFFFFFFF
f32 = np.float32


def wave(tris, amp, frame):
    """main.js --animate AMP at `frame`: every vertex moves in y by AMP times a triangle wave of its own x, every step rounded to f32:
    u = ((2 x + 0.25) + 0.125 frame); y += AMP (4 |u - floor(u) - 0.5| - 1).  Add, multiply, floor, abs only."""
    v = np.array(tris, f32).reshape(-1, 3)
    x = v[:, 0]
    u = ((f32(2) * x).astype(f32) + f32(0.25)).astype(f32) + f32(f32(0.125) * f32(frame))
    d = ((u - np.floor(u)).astype(f32) - f32(0.5)).astype(f32)
    tri = ((f32(4) * np.abs(d)).astype(f32) - f32(1)).astype(f32)
    v[:, 1] = (v[:, 1] + (f32(amp) * tri).astype(f32)).astype(f32)
    return v.reshape(-1)


def ord16(bits):
    """f16 bits -> an integer that orders like the value (-0 just below +0)."""
    bits = np.asarray(bits, np.int64)
    return np.where(bits & 0x8000, (~bits) & 0xFFFF, bits ^ 0x8000)


def unord16(o):
    o = np.asarray(o, np.int64)
    return np.where(o & 0x8000, o ^ 0x8000, (~o) & 0xFFFF) & 0xFFFF


def halves(words):
    """(.., 3) box words -> (.., 6) f16 bit patterns: mn.x mn.y mn.z mx.x mx.y mx.z"""
    w = np.asarray(words, np.int64)
    return np.stack([w[..., 0] & 0xFFFF, w[..., 0] >> 16, w[..., 1] & 0xFFFF, w[..., 1] >> 16, w[..., 2] & 0xFFFF, w[..., 2] >> 16], -1)


def pack(h):
    h = np.asarray(h, np.int64)
    return np.stack([h[..., 0] | (h[..., 1] << 16), h[..., 2] | (h[..., 3] << 16), h[..., 4] | (h[..., 5] << 16)], -1).astype(np.uint32)


def leaf_boxes(tris, t):
    """The leaf rule for triangles t: min / max of the three vertices (no NaN here; -0 below +0), round-to-nearest-even to f16, then one f16
    step outwards, always (BVHBuilder.wgsl:63-102).  Returns (len(t), 3) words."""
    v = np.asarray(tris, f32).reshape(-1, 3, 3)[t]
    # numpy's float16 cast rounds to nearest even; in the ordered integer form min / max respect the sign of zero and a step is +-1
    o = ord16(v.astype(np.float16).view(np.uint16))
    lo, hi = o.min(1) - 1, o.max(1) + 1
    # rounding is monotone, so min / max commute with it -- except that f32 values which differ only in the sign of zero, or round to the
    # same f16, are ordered before the rounding on the device; both give the same f16 result
    return pack(unord16(np.concatenate([lo, hi], -1)))


def numpy_refit_bvh4(tris, bvh4):
    """The three BVH4 rules for a tree whose children have larger ids than their parent (every tree this library builds)."""
    out = np.array(bvh4, np.uint32)
    m = int(out[0])
    n = np.asarray(tris).size // 9
    rec = out[1:1 + 8 * m].reshape(m, 8)
    leaf = (rec[:, 7] & LEAF) != 0
    t = (rec[:, 7] & 0x7FFFFFFF).astype(np.int64)
    sel = np.nonzero(leaf & (t < n))[0]
    rec[sel, :3] = leaf_boxes(tris, t[sel])
    o = ord16(halves(rec[:, :3]))
    inf_lo, inf_hi = int(ord16(0x7C00)), int(ord16(0xFC00))
    for i in np.nonzero(~leaf)[0][::-1]:
        kids = [int(c) for c in rec[i, 3:7] if c != INVALID and c < m]
        if not kids:
            continue
        assert min(kids) > i
        ko = o[kids]
        box = np.concatenate([np.minimum(ko[:, :3].min(0), inf_lo), np.maximum(ko[:, 3:].max(0), inf_hi)])
        h = unord16(box)
        h = np.where((h & 0x7C00) == 0, h & 0x8000, h)          # PathTracer.js:42-51: below the f16 normal range -> signed zero
        o[i] = ord16(h)
        rec[i, :3] = pack(h)
    return out


def numpy_cost(bvh4):
    """Sum over internal nodes reachable from the root of halfArea(node) / halfArea(root), exactly decoded bounds, f64."""
    b = np.asarray(bvh4, np.uint32)
    m = int(b[0])
    if m == 0:
        return 0.0
    rec = b[1:1 + 8 * m].reshape(m, 8)
    seen = np.zeros(m, bool)
    stack = [0]
    seen[0] = True
    while stack:
        i = stack.pop()
        if rec[i, 7] & LEAF:
            continue
        for c in rec[i, 3:7]:
            if c != INVALID and c < m:
                assert not seen[c]
                seen[c] = True
                stack.append(int(c))
    h = halves(rec[:, :3]).astype(np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.all(h[:, :3] <= h[:, 3:], -1)
        d = h[:, 3:] - h[:, :3]
        area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    area = np.where(ok & ~np.isnan(area), area, 0.0)
    if not (area[0] > 0 and np.isfinite(area[0])):
        return 0.0
    terms = area[seen & ((rec[:, 7] & LEAF) == 0)] / area[0]
    return float(np.sum(terms))


def host_trees(rt, orc, tris, accel):
    """(BVH2, BVH4) of build level `accel` from the host twins of the build."""
    n = np.asarray(tris).size // 9
    b2 = rt.build_bvh2_ploc(tris) if accel == rt.PT_ACCEL_PLOC else orc.build_lbvh2(tris)
    return b2, rt.collapse_bvh2_to_bvh4_accel(b2, n, accel)[0]


def check_refit_invariants(before, after):
    """Topology words untouched; every internal box contains its children's (up to the subnormal flush of PathTracer.js:42-51)."""
    b, a = np.asarray(before, np.uint32), np.asarray(after, np.uint32)
    m = int(a[0])
    assert a[0] == b[0] and len(a) == len(b)
    ra, rb = a[1:1 + 8 * m].reshape(m, 8), b[1:1 + 8 * m].reshape(m, 8)
    assert np.array_equal(ra[:, 3:], rb[:, 3:])
    h = halves(ra[:, :3]).astype(np.uint16).view(np.float16).astype(np.float32)
    tiny = f32(2.0 ** -14)
    for s in range(4):
        c = ra[:, 3 + s]
        sel = (c != INVALID) & (c < m) & ((ra[:, 7] & LEAF) == 0)
        k = c[sel].astype(np.int64)
        assert np.all((h[sel, :3] <= h[k, :3]) | ((np.abs(h[k, :3]) < tiny) & (h[sel, :3] == 0)))
        assert np.all((h[sel, 3:] >= h[k, 3:]) | ((np.abs(h[k, 3:]) < tiny) & (h[sel, 3:] == 0)))
