"""The tile cover restated in numpy float64: which 8x8 tiles of a frame a launch has to trace.

Written from the design, not from pt_cover.hip, and it does not import the package.  Input: the words of read_bvh4() (or of
orc.build_bvh4): a count, then 8 words per node -- 3 words of f16 box, 4 children, meta -- and anything with the fields width, height,
focal, aspect, cam_pos, cam_quat (the package's render params, the oracle's).

  cut(bvh4)                   the breadth-first cut: the nodes whose boxes are projected
  screen_rect(boxes, params)  eight corners per box through the camera model of the root box's rectangle
  root_rect(bvh4, params, m)  the root box's tile rectangle as a mask, None where every tile is traced
  cover(bvh4, params, m)      the union of the cut's tile rectangles inside the root's, None where the launch keeps the rectangle
  expected(bvh4, params)      (inner, outer): the cover at margins 2 - 1e-6 and 2 + 1e-6 px.  The device projects in f64 but may
                              contract a multiply and an add into one rounding, so a box edge within 1e-6 px of a tile seam may fall
                              either way; everything else has to be equal: inner <= device <= outer
  cameras(rng, n, extent)     the seeded views every cover test uses

Test helper, not product code and not a conftest."""
import numpy as np

from refit_cases import INVALID, LEAF
from treeaudit import decode

TILE = 8
CUT_MAX = 4096          # the cut is the last level of the breadth-first walk with at most this many entries ...
CUT_LEVELS = 64         # ... and the walk takes at most this many steps down
MARGIN = 2.0            # px added around every projected box
BAND = 1e-6             # px: see expected()
NEAR = 1e-4             # a corner with view-space z >= -NEAR is beside or behind the eye


def _records(bvh4):
    w = np.asarray(bvh4, np.uint32)
    m = int(w[0]) if len(w) else 0
    return m, w[1:1 + 8 * m].reshape(m, 8)


def _empty(boxes):
    """any(mn > mx): no ray enters it (false when a NaN is involved)."""
    with np.errstate(invalid="ignore"):
        return (boxes[..., :3] > boxes[..., 3:]).any(-1)


def cut(bvh4):
    """Node indices of the cut, or None when there is none (empty tree, or the root is a leaf).  The frontier starts as the root's
    children.  A step replaces every internal entry by its children and keeps a leaf; a child word that is INVALID, or names no node,
    is never an entry; an entry whose box is inverted stays as it is (no ray enters it: nothing below it is reached).  The cut is the
    last frontier of at most CUT_MAX entries: the walk also ends when nothing expands, or after CUT_LEVELS steps."""
    m, rec = _records(bvh4)
    if m == 0 or rec[0, 7] & LEAF:
        return None
    kids = rec[:, 3:7].astype(np.int64)
    ok = (kids != INVALID) & (kids < m)
    stays = ((rec[:, 7] & LEAF) != 0) | _empty(decode(rec[:, :3]))
    front = kids[0][ok[0]]
    for _ in range(CUT_LEVELS):
        grow = ~stays[front]
        if not grow.any():
            break
        inner = front[grow]
        nxt = np.concatenate([front[~grow], kids[inner][ok[inner]]])
        if len(nxt) > CUT_MAX:
            break
        front = nxt
    return front


def screen_rect(boxes, params):
    """(n, 6) boxes (mn.xyz, mx.xyz) -> (rect (n, 4): min x, max x, min y, max y in pixels; bad (n,); empty (n,)).  v = conj(q) p q takes
    a corner into the camera's frame (the camera looks down -z), sx = vx / -vz focal / aspect, sy = vy / -vz focal,
    fx = (sx + 1) / 2 width, fy likewise.  bad: a corner beside or behind the eye, or a value that is not finite -- such a box has no
    screen rectangle.  empty: any(mn > mx) -- it covers nothing, whatever else it holds."""
    b = np.asarray(boxes, np.float64).reshape(-1, 6)
    q = np.array([float(v) for v in params.cam_quat], np.float64)
    cam = np.array([float(v) for v in params.cam_pos], np.float64)
    focal, aspect = float(params.focal), float(params.aspect)
    pick = np.array([[(k >> a) & 1 for a in range(3)] for k in range(8)], bool)            # corner k takes mx on axis a when bit a is set
    p = np.where(pick[None], b[:, None, 3:], b[:, None, :3]) - cam                         # (n, 8, 3)
    (ux, uy, uz), s = -q[:3], q[3]
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        cx, cy, cz = uy * pz - uz * py, uz * px - ux * pz, ux * py - uy * px                # c = u x p
        vx = px + 2.0 * (s * cx + (uy * cz - uz * cy))                                     # v = p + 2 (s c + u x c)
        vy = py + 2.0 * (s * cy + (uz * cx - ux * cz))
        vz = pz + 2.0 * (s * cz + (ux * cy - uy * cx))
        fx = (vx / -vz * focal / aspect + 1.0) * 0.5 * float(params.width)
        fy = (vy / -vz * focal + 1.0) * 0.5 * float(params.height)
        good = (vz < -NEAR) & (np.abs(fx) < 1e300) & (np.abs(fy) < 1e300)                  # a NaN fails every compare
        rect = np.stack([fx.min(1), fx.max(1), fy.min(1), fy.max(1)], -1)
    empty = _empty(b)
    return rect, ~good.all(1) & ~empty, empty


def _tiles(params):
    return (int(params.width) + TILE - 1) // TILE, (int(params.height) + TILE - 1) // TILE


def _tile_union(rect, tiles_x, tiles_y, margin):
    """Union of the tile rectangles [lo, hi) of the pixel rectangles, lo = floor((v - margin) / 8), hi = floor((v + margin) / 8 + 1), clamped to the frame."""
    def lo(v, n): return np.clip(np.floor((v - margin) / TILE), 0, n)
    def hi(v, n): return np.clip(np.floor((v + margin) / TILE + 1.0), 0, n)
    tx, ty = np.arange(tiles_x), np.arange(tiles_y)
    X = (tx >= lo(rect[:, 0], tiles_x)[:, None]) & (tx < hi(rect[:, 1], tiles_x)[:, None])
    Y = (ty >= lo(rect[:, 2], tiles_y)[:, None]) & (ty < hi(rect[:, 3], tiles_y)[:, None])
    return (Y.T.astype(np.int64) @ X.astype(np.int64)) > 0


_PREPARED = {}


def _prepared(bvh4):
    """(node count, the root's box, the boxes of the cut or None) of these words; the last few trees are kept, by content."""
    w = np.ascontiguousarray(bvh4, np.uint32)
    key = hash(w.tobytes())
    if key not in _PREPARED:
        if len(_PREPARED) >= 8:
            _PREPARED.pop(next(iter(_PREPARED)))
        m, rec = _records(w)
        entries = cut(w)
        _PREPARED[key] = (m, decode(rec[:1, :3]) if m else None, None if entries is None else decode(rec[entries, :3]))
    return _PREPARED[key]


class _Projection:
    """Everything about (tree, camera) that does not depend on the margin."""

    def __init__(self, bvh4, params, with_cut=True):
        m, root, boxes = _prepared(bvh4)
        self.tiles = _tiles(params)
        self.root = self.rects = None
        q = np.array([float(v) for v in params.cam_quat], np.float64)
        if m == 0 or not (abs(float((q * q).sum()) - 1.0) < 1e-5 and float(params.focal) > 1e-3 and float(params.aspect) > 1e-3):
            return
        rect, bad, empty = screen_rect(root, params)
        if bad[0] or empty[0]:
            return
        self.root = rect
        if with_cut and boxes is not None:
            rect, bad, empty = screen_rect(boxes, params)
            if not bad.any():
                self.rects = rect[~empty]

    def root_rect(self, margin):
        return None if self.root is None else _tile_union(self.root, *self.tiles, margin)

    def cover(self, margin):
        return None if self.rects is None else _tile_union(self.rects, *self.tiles, margin) & self.root_rect(margin)


def root_rect(bvh4, params, margin=MARGIN):
    """The root box's tile rectangle as a bool mask [tiles_y, tiles_x], or None where a launch leaves out nothing: no tree, a root box
    that is inverted or has a corner beside the eye, a quaternion whose squared length is not within 1e-5 of 1, a focal length or an
    aspect ratio that is not above 1e-3."""
    return _Projection(bvh4, params, with_cut=False).root_rect(margin)


def cover(bvh4, params, margin=MARGIN):
    """The tiles a launch traces under the cover, bool [tiles_y, tiles_x]: the union of the tile rectangles of the cut's boxes, inside the
    root box's rectangle at the same margin.  None for "no cover": the launch keeps the rectangle (or, without one, every tile) because
    there is no cut, no rectangle, or one box of the cut has no screen rectangle."""
    return _Projection(bvh4, params).cover(margin)


def covers(bvh4, params, margins):
    """cover() at several margins from one projection."""
    pr = _Projection(bvh4, params)
    return [pr.cover(m) for m in margins]


def expected(bvh4, params):
    """(inner, outer): what the device's mask has to contain and what has to contain it; (None, None) for "no cover"."""
    inner, outer = covers(bvh4, params, (MARGIN - BAND, MARGIN + BAND))
    return inner, outer


def _qmul(a, b):
    """Hamilton product, xyzw."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def cameras(rng, n, extent, centre=(0.0, 0.0, 0.0)):
    """n views as (position, quaternion xyzw), both rounded to f32.  `extent`: the longest side of the scene's box.  The position lies on
    a shell of radius 1.2 - 5 extents around the centre in a uniform direction; every fifth one at 0.3 - 1.2 extents instead, where the
    root box or a box of the cut comes beside the eye and the rectangle, or every tile, has to come back.  The view is aimed at the
    centre, then turned by normal jitter of 0.25 rad in yaw and 0.2 rad in pitch -- part of the scene leaves the frame -- and rolled
    about its axis by a uniform angle in +-pi.  q = yaw(Y) pitch(X) roll(Z), normalised in f64, rounded to f32: |q|^2 is within 1e-6 of 1."""
    out = []
    centre = np.asarray(centre, np.float64)
    for i in range(n):
        d = rng.normal(size=3)
        d /= np.sqrt((d * d).sum())
        r = extent * (rng.uniform(0.3, 1.2) if i % 5 == 4 else rng.uniform(1.2, 5.0))
        pos = (centre + r * d).astype(np.float32)
        f = -d                                                  # forward; q takes (0, 0, -1) to (-sin yaw cos pitch, sin pitch, -cos yaw cos pitch)
        yaw = np.arctan2(-f[0], -f[2]) + rng.normal(0.0, 0.25)
        pitch = np.arcsin(np.clip(f[1], -1.0, 1.0)) + rng.normal(0.0, 0.2)
        roll = rng.uniform(-np.pi, np.pi)
        q = _qmul(_qmul([0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)], [np.sin(pitch / 2), 0.0, 0.0, np.cos(pitch / 2)]), [0.0, 0.0, np.sin(roll / 2), np.cos(roll / 2)])
        q = (q / np.sqrt((q * q).sum())).astype(np.float32)
        out.append((tuple(float(v) for v in pos), tuple(float(v) for v in q)))
    return out


def extent_of(bvh4):
    """The longest side of the root box."""
    _, rec = _records(bvh4)
    b = decode(rec[0, :3])
    return float((b[3:] - b[:3]).max())


def hit_tiles(hit, width, height):
    """[height, width] bool -> the tiles that hold a True pixel."""
    t = np.zeros(((height + TILE - 1) // TILE, (width + TILE - 1) // TILE), bool)
    ys, xs = np.nonzero(hit)
    t[ys // TILE, xs // TILE] = True
    return t
