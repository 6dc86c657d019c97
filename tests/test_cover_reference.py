"""tests/coverref.py -- the float64 restatement of the tile cover -- against the CPU oracle, before it judges the
device (tests/test_gpu_tile_cover_sweep.py): a cover has to hold every tile in which the oracle hits anything, from every camera of the
seeded generator, on four trees that each bind another rule of the cut; and the check has to be able to fail.  No GPU."""
import functools

import numpy as np
import pytest

import coverref
import orc as orc_mod
from scenes import comb_bvh4, random_soup, spoil_bvh4

RES = [(200, 120), (250, 141), (64, 40)]
MISS = 0xFFFFFFFF
# cameras per tree (the oracle needs several times as long per frame on the comb: every ray walks the whole chain), and how many of them also get a MODE_PATH frame
CAMERAS = {"soup300": 96, "soup6000": 84, "spoiled": 84, "comb": 80}
PATH_CAMERAS = 12
PATH = dict(spp=4, max_bounces=1, seed=9)
TREES = list(CAMERAS)


@functools.lru_cache(maxsize=None)
def tree(name):
    """(tris, bvh4) -- read-only, shared."""
    orc = orc_mod.load()
    if name == "comb":
        tris, b = comb_bvh4(90, 2, all_hit=False)
    else:
        tris = random_soup(300 if name == "soup300" else 6000, 3)
        b = orc.build_bvh4(tris)[1]
        if name == "spoiled":
            b = spoil_bvh4(b, 5)[0]
    tris.setflags(write=False); b.setflags(write=False)
    return tris, b


def degenerate_in_cut(b):
    rec = np.asarray(b[1:]).reshape(-1, 8)
    box = coverref.decode(rec[coverref.cut(b), :3])
    return int((box[:, :3] > box[:, 3:]).any(1).sum())


def traced(mask, rect, params):
    """What a launch traces: the cover, the rectangle where there is none, every tile where there is no rectangle either."""
    if mask is not None:
        return mask
    tx, ty = coverref._tiles(params)
    return rect if rect is not None else np.ones((ty, tx), bool)


def render_ids(orc, params, tris, bvh4, band=8):
    """The triangle ids of a MODE_SINGLE frame, rendered in strips of rows on several threads like orc.render_mt (the C call releases the GIL)."""
    import ctypes as C
    import os
    from concurrent.futures import ThreadPoolExecutor
    ids = np.full((params.height, params.width), MISS, np.uint32)
    img = np.zeros((params.height, params.width, 4), np.float32)

    def work(y):
        p = orc_mod.Params.from_buffer_copy(params)
        p.y0, p.y1 = y, min(y + band, params.height)
        st = orc_mod.Stats()
        assert orc.lib.orc_render(C.byref(p), orc_mod._p(tris, C.c_float), orc_mod._p(bvh4, C.c_uint32), orc_mod._p(img, C.c_float), orc_mod._p(ids, C.c_uint32), C.byref(st)) == 0

    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as ex:
        list(ex.map(work, range(0, params.height, band)))
    return ids


@functools.lru_cache(maxsize=None)
def miss_value():
    """The MODE_PATH value of a pixel none of whose samples hits anything: a frame that looks away from the scene."""
    orc = orc_mod.load()
    tris, b = tree("soup300")
    img, _, _ = orc.render(orc.make_params(16, 8, tris.size // 9, (0, 0, 50), (0, 1, 0, 0), mode=orc_mod.MODE_PATH, **PATH), tris, b)
    assert (img.reshape(-1, 4) == img[0, 0]).all()
    return img[0, 0].copy()


@functools.lru_cache(maxsize=None)
def sweep(name):
    """One pass over the tree's cameras, shared by the tests: per camera the oracle's hit tiles and the reference's answers."""
    orc = orc_mod.load()
    tris, b = tree(name)
    rows = []
    cams = coverref.cameras(np.random.default_rng(1000 + TREES.index(name)), CAMERAS[name], coverref.extent_of(b))
    for i, (pos, quat) in enumerate(cams):
        w, h = RES[i % 3]
        p = orc.make_params(w, h, tris.size // 9, pos, quat, mode=orc_mod.MODE_SINGLE)
        ids = render_ids(orc, p, tris, b)
        r = dict(i=i, w=w, h=h, params=p, hits=coverref.hit_tiles(ids != MISS, w, h), rect=coverref.root_rect(b, p))
        r["inner"], r["outer"], r["plain"], r["short"] = coverref.covers(b, p, (coverref.MARGIN - coverref.BAND, coverref.MARGIN + coverref.BAND, 0.0, -8.0))
        if i < PATH_CAMERAS:
            pp = orc.make_params(w, h, tris.size // 9, pos, quat, mode=orc_mod.MODE_PATH, **PATH)
            img = orc.render_mt(pp, tris, b)[0]
            r["lit"] = coverref.hit_tiles((img != miss_value()).any(-1), w, h)
        rows.append(r)
    return rows


def test_cut_sizes():
    """All leaves; the 4,096 cap binds (the next level has more); inverted boxes among the entries; 3 x 64 + 4: the 64-step stop binds."""
    sizes = {n: len(coverref.cut(tree(n)[1])) for n in TREES}
    deg = degenerate_in_cut(tree("spoiled")[1])
    print("cut entries %s, inverted boxes in the spoiled tree's cut %d" % (sizes, deg))
    assert sizes["soup300"] == 300 and sizes["soup6000"] == 3932 and sizes["comb"] == 196
    assert deg >= 5 and degenerate_in_cut(tree("soup6000")[1]) == 0
    leaf = np.zeros(9, np.uint32); leaf[0] = 1; leaf[8] = 0x80000000
    assert coverref.cut(leaf) is None and coverref.cut(np.zeros(1, np.uint32)) is None


@pytest.mark.parametrize("name", TREES)
def test_cover_holds_every_hit(name):
    """Every tile with a MODE_SINGLE hit (every pixel centre) lies in the inner cover -- and in the cover without any margin; on a dozen
    cameras so does every tile with a MODE_PATH pixel that differs from the miss value (jittered samples, a bounce).  The band between the
    inner and the outer cover is empty on at least 99 % of the cameras."""
    rows = sweep(name)
    out1 = sum(int((r["hits"] & ~traced(r["inner"], r["rect"], r["params"])).sum()) for r in rows)
    out0 = sum(int((r["hits"] & ~traced(r["plain"], r["rect"], r["params"])).sum()) for r in rows)
    out2 = sum(int((r["lit"] & ~traced(r["inner"], r["rect"], r["params"])).sum()) for r in rows if "lit" in r)
    lit = sum(int(r["lit"].sum()) for r in rows if "lit" in r)
    band = sum(1 for r in rows if r["inner"] is not None and not np.array_equal(r["inner"], r["outer"]))
    print("%s: %d cameras, hit tiles outside the cover %d (margin 2), %d (margin 0); MODE_PATH tiles %d, outside %d; inner != outer on %d cameras" % (name, len(rows), out1, out0, lit, out2, band))
    assert out1 == 0 and out2 == 0 and lit > 0
    assert band * 100 <= len(rows)
    for r in rows:
        if r["inner"] is not None:
            assert not (r["inner"] & ~r["outer"]).any() and not (r["outer"] & ~r["rect"]).any()


@pytest.mark.parametrize("name", TREES)
def test_cover_is_not_vacuous_and_the_check_has_teeth(name):
    """On at least half the cameras of each tree: a tile holds a hit; the cover is a proper subset of the rectangle; and the same cover at
    margin -8 px (every box one tile short on each side) loses a tile with a hit -- a cover that is too small does not pass."""
    rows = sweep(name)
    n = len(rows)
    have = [r for r in rows if r["inner"] is not None]
    hit = sum(1 for r in rows if r["hits"].any())
    proper = sum(1 for r in have if int(r["outer"].sum()) < int(r["rect"].sum()))
    lost = sum(1 for r in have if (r["hits"] & ~r["short"]).any())
    norect = sum(1 for r in rows if r["rect"] is None)
    print("%s: %d cameras: no rectangle %d, rectangle but no cover %d; a hit tile on %d, cover < rectangle on %d, margin -8 loses a hit tile on %d" % (
        name, n, norect, n - len(have) - norect, hit, proper, lost))
    assert 2 * hit >= n and 2 * proper >= n and 2 * lost >= n
    assert norect > 0                      # the near shell does what it is there for
