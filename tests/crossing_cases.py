"""Shared by the crossing-query tests (tests/test_crossings_host.py, tests/test_gpu_crossings.py, tests/crossings_torch_cases.py):
the scenes, their trees, the ray and point sets, and the composition that pt_contains is specified as."""
import numpy as np

from refit_cases import host_trees, wave
from scenes import TETRA, closed_box, comb_bvh4, cornell, random_soup, spoil_bvh4

SCENE_SEED = 20260109
MISS = 0xFFFFFFFF
CLOSED = ["tetra", "box", "torus"]                                   # point-in-solid has a meaning here
SCENES = ["tetra", "box", "cornell", "soup1k", "dragon50k", "torus"]
COMB_LEVELS, COMB_SEED = 30, 5


def torus(nu=48, nv=24, major=0.7, minor=0.25):
    """A closed genus-1 mesh, nu x nv quads = 2 * nu * nv triangles over shared vertices (watertight: neighbours use the same floats):
    y scaled by 0.8 and offset by 0.1 cos v, z offset by 0.05 sin 3u, so that nothing is axis-aligned."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    ring = major + minor * np.cos(V)
    P = np.stack([ring * np.cos(U), 0.8 * ring * np.sin(U) + 0.1 * np.cos(V), minor * np.sin(V) + 0.05 * np.sin(3 * U)], axis=2).astype(np.float32)
    out = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = P[i, j], P[(i + 1) % nu, j], P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
            out += [a, b, c, a, c, d]
    tris = np.array(out, np.float32).reshape(-1)
    assert tris.size == 9 * 2 * nu * nv
    return tris


def geometry(rt, name):
    if name == "tetra":
        return TETRA
    if name == "box":
        return closed_box()
    if name == "cornell":
        return cornell()[0]
    if name == "soup1k":
        return random_soup(1000, 3)
    if name == "dragon50k":
        return rt.procedural_scene(rt.SCENE_DRAGON_CLASS, 50000, SCENE_SEED)
    if name == "comb":
        return comb_bvh4(COMB_LEVELS, COMB_SEED)[0]
    if name == "spoiled":
        return random_soup(3000, 23)
    assert name == "torus"
    return torus()


def comb_tree():
    return comb_bvh4(COMB_LEVELS, COMB_SEED)[1]


def spoiled_tree(rt, orc, tris):
    b4, n_oob, n_deg = spoil_bvh4(host_trees(rt, orc, tris, 0)[1], 9)
    assert n_oob > 0 and n_deg > 0
    return b4


def forest(rt, orc, tris):
    """[(label, triangles, bvh4)]: the three build levels over `tris`, and the level-0 topology refitted to displaced vertices."""
    out = [("accel%d" % a, tris, host_trees(rt, orc, tris, a)[1]) for a in (0, 1, 2)]
    moved = wave(tris, 0.02, 3)
    out.append(("accel0+refit", moved, rt.refit_bvh4(moved, out[0][2])))
    return out


def surfels_of(points):
    """The surfels whose occlusion rays are the containment rays: {p, r_max = +inf, n = (0, 0, 1)}."""
    p = np.asarray(points, np.float32)
    p = p.reshape(-1, p.shape[-1])[:, :3]                               # (n, 3) points or (n, 4) PtPoint records
    sf = np.zeros((len(p), 8), np.float32)
    sf[:, 0:3] = p; sf[:, 3] = np.inf; sf[:, 6] = 1.0
    return sf


def containment_rays(rt, points, samples, seed=0, index_base=0):
    return rt.occlusion_rays_host(surfels_of(points), samples, seed=seed, bias=0.0, index_base=index_base)


def box_of(tris):
    v = np.asarray(tris, np.float32).reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def ray_set(rt, tris, n, seed):
    """n PtRay records: half from random origins in 1.5 x the box toward random points of the box (direction = target - origin, not
    normalised; a quarter of them end at the target, t_max = 1), half the containment rays of random points in 1.2 x the box."""
    rng = np.random.default_rng(seed)
    lo, hi = box_of(tris)
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    k = n // 2
    org = (c + (rng.random((k, 3)) * 2 - 1) * 1.5 * h).astype(np.float32)
    tgt = (c + (rng.random((k, 3)) * 2 - 1) * h).astype(np.float32)
    t_max = np.where(np.arange(k) % 4 == 3, np.float32(1.0), np.float32(np.inf))
    aimed = rt.pack_rays(org, tgt - org, t_max)
    pts = (c + (rng.random((n - k, 3)) * 2 - 1) * 1.2 * h).astype(np.float32)
    out = rt.pack_rays(np.zeros((n, 3)), np.zeros((n, 3)))
    out[:k] = aimed
    out[k:] = containment_rays(rt, pts, 1, seed=seed)
    return out


def comb_rays(rt, n, seed):
    """Rays down -z from in front of the comb: they pass every level, so the walk runs into the 64-entry cap."""
    rng = np.random.default_rng(seed)
    org = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), np.full(n, 2.0)], axis=1).astype(np.float32)
    d = np.stack([rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n), np.full(n, -1.0)], axis=1).astype(np.float32)
    return rt.pack_rays(org, d)


def cube_points(n, seed, half=1.2):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32)


def compose_contains(odd_per_ray, n, samples):
    """parity -> majority: (inside, odd, samples) from the n * samples ray counts."""
    odd = (np.asarray(odd_per_ray).reshape(n, samples) & 1).sum(axis=1).astype(np.uint32)
    return (2 * odd > samples).astype(np.uint32), odd, np.full(n, samples, np.uint32)
