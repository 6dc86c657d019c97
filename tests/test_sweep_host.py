"""Sphere-cast queries on the CPU: the host twin pt_sweep_spheres_bvh4 (include/mi355pt.h) against the numpy-float32
restatement of csrc/pt_sweep.h (tests/sweep_cases.py) bit for bit, the tree walk against brute force (both on the twin), and the twin
against the independent float64 reference (tests/sweepref.py) through a sandwich in the radius.  The GPU tests (tests/test_gpu_sweep.py)
pin the kernels to this twin word for word.

Measured here (MEASURED_K, the wide shares and the deepest stacks are repeated in DESIGN.md section 22):
  smallest K at which the twin passes the sandwich on every scene and tree: see sweep_cases.MEASURED_K
  wide sandwiches at TOL_K, of the items of each scene: printed by test_sandwich_against_float64
  deepest stack per scene and tree: printed by test_walk_equals_brute_force"""
import ctypes as C
import functools

import numpy as np
import pytest

import crossing_cases as xc
import sweep_cases as sc
from scenes import comb_bvh4

PT_ERR_INVALID_ARG, PT_ERR_BAD_BVH = 1, 5        # include/mi355pt.h PtStatus
SCENES = ["tetra", "box", "cornell", "soup1k", "torus", "dragon50k"]
ITEMS = {"tetra": 1500, "box": 1500, "cornell": 1500, "soup1k": 1024, "torus": 768, "dragon50k": 64}      # every triangle for every item, in float64
f32 = np.float32


class Case:
    """One scene with one geometry (as built, or displaced for the refit): the sweeps, the brute-force twin and the float64 band, computed
    once and shared by the tests below, which leave them unchanged."""

    def __init__(self, rt, name, moved):
        base = xc.geometry(rt, name)
        self.tris = xc.wave(base, 0.02, 3) if moved else base
        self.sweeps = sc.sweep_set(rt, self.tris, ITEMS[name], 11 + moved)
        self.brute = rt.sweep_spheres_bvh4(self.tris, None, self.sweeps, brute_force=True)

    @functools.cached_property
    def band(self):
        return sc.reference_band(self.sweeps, self.tris)


@functools.lru_cache(maxsize=None)
def _case(rt, name, moved):
    return Case(rt, name, moved)


@pytest.mark.parametrize("name", SCENES)
def test_brute_twin_equals_numpy_restatement(rt, name):
    for moved in (False, True):
        c = _case(rt, name, moved)
        prod = sc.product_sweep(c.sweeps, c.tris)
        sc.check_same_minimum(c.sweeps, c.tris, c.brute, prod)
        assert np.array_equal(c.brute[1], prod[1])                       # both take the first minimum in index order


@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_brute_force(rt, orc, name):
    """Levels 0-2 over the geometry as built, and the level-0 topology refitted to the displaced vertices: t, u, v bit for bit, prim up to
    ties of t_T, nothing dropped at the cap."""
    base = xc.geometry(rt, name)
    for label, tris, b4 in xc.forest(rt, orc, base):
        c = _case(rt, name, tris is not base)
        assert np.array_equal(c.tris, tris)
        res = rt.sweep_spheres_bvh4(tris, b4, c.sweeps, stats=True)
        st = res[4]
        print("sweep %s %s: deepest stack %d, %.1f node records and %.2f triangles per item" % (
            name, label, st["max_stack"], st["nodes_examined"] / len(c.sweeps), st["tris_tested"] / len(c.sweeps)))
        assert st["rays_closest"] == len(c.sweeps) and st["stack_drops"] == 0 and 1 <= st["max_stack"] <= 64, (label, st)
        sc.check_same_minimum(c.sweeps, tris, res[:4], c.brute)
        sc.check_uv(c.sweeps, tris, res[:4])
        plain = rt.sweep_spheres_bvh4(tris, b4, c.sweeps, simple=True)                    # no counters, the flag changes nothing
        assert all(sc.same_bits(a, b) for a, b in zip(plain, res[:4]))


@pytest.mark.parametrize("name", SCENES)
def test_sandwich_against_float64(rt, name):
    """t_ref(r + tol) - tau <= t <= t_ref(max(r - tol, 0)) + tau on every item, no item excluded (sweep_cases.sandwich_violation).  The
    walks equal brute force bit for bit (test_walk_equals_brute_force), so the brute-force twin stands for every tree."""
    for moved in (False, True):
        c = _case(rt, name, moved)
        wide = c.band[3]
        print("sweep %s%s: %d of %d sandwiches wide at K = %g" % (name, "+refit" if moved else "", int(wide.sum()), len(wide), sc.TOL_K))
        assert wide.mean() <= sc.WIDE_SHARE, int(wide.sum())                              # on the reference alone
        worst = sc.sandwich_violation(c.sweeps, c.tris, c.brute[0], c.band)
        assert worst <= 0.0, worst


@pytest.mark.parametrize("name", SCENES)
def test_clearance_at_the_reported_time(rt, name):
    """The centre at the reported time touches the mesh: within [r - tol, r + tol] of it where the sphere had to move (t > 0), and within
    r + tol where it overlapped at the start (t = 0: a sphere that starts deep inside the surface is nearer than r, so there is no lower
    side to check)."""
    for moved in (False, True):
        c = _case(rt, name, moved)
        t, prim = c.brute[0], c.brute[1]
        hit = prim != sc.MISS
        centre = sc.contact_point(c.sweeps[hit], t[hit])
        dist = rt.closest_points_bvh4(c.tris, None, centre, brute_force=True)[0].astype(np.float64)
        r = c.sweeps[hit, 7].astype(np.float64)
        tol = sc.TOL_K * sc.units(c.sweeps, c.tris)[hit]
        later = t[hit] > 0
        dev = (dist - r) / tol * sc.TOL_K
        print("sweep %s%s: clearance at t > 0 within [%.3g, %.3g] units of r" % (name, "+refit" if moved else "", float(dev[later].min()), float(dev[later].max())))
        assert np.all(dist[later] >= (r - tol)[later])
        assert np.all(dist <= r + tol)


@pytest.mark.parametrize("name", SCENES)
def test_overlap_at_the_start_is_time_zero(rt, name):
    """Every item for which the radius query lists a triangle within r of the origin hits at t <= tau."""
    c = _case(rt, name, False)
    off = rt.radius_search_bvh4(c.tris, None, c.sweeps[:, 0:3], r_max=c.sweeps[:, 7], brute_force=True)[0]
    listed = np.diff(off.astype(np.int64)) > 0
    assert listed.any() or ITEMS[name] < 100
    S = c.sweeps.astype(np.float64)
    tau = sc.TOL_K * sc.units(c.sweeps, c.tris) / np.linalg.norm(S[:, 4:7], axis=1)
    assert np.all(c.brute[1][listed] != sc.MISS) and np.all(c.brute[0][listed] <= tau[listed])


@pytest.mark.parametrize("name", SCENES)
def test_contact_uv_is_the_closest_point_arithmetic(rt, name):
    c = _case(rt, name, False)
    sc.check_uv(c.sweeps, c.tris, c.brute)


UNIT = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], f32)          # the triangle (0,0,0), (1,0,0), (0,1,0)
EXACT = [
    # origin, direction, radius, expected t (None: a miss), expected (u, v)
    ("face from above", (0.25, 0.25, 2), (0, 0, -1), 0.5, 1.5, (0.25, 0.25)),            # the plane z = 0 moved up by r: (2 - 0.5) / 1
    ("edge from the side, in the plane", (0.5, -2, 0), (0, 1, 0), 0.5, 1.5, (0.5, 0.0)),  # the edge y = 0 reached at y = -0.5
    ("vertex", (4, 0, 0), (-1, 0, 0), 1.0, 2.0, (1.0, 0.0)),                             # the vertex (1, 0, 0) reached at x = 2
    ("overlapping at the start", (0.25, 0.25, 0.25), (0, 0, 1), 0.5, 0.0, (0.25, 0.25)),
    ("moving away", (0.25, 0.25, 2), (0, 0, 1), 0.5, None, None),
    ("grazing pass at r + 2^-20", (-2, 0.5, 0.5 + 2.0 ** -20), (1, 0, 0), 0.5, None, None),
]


@pytest.mark.parametrize("case", EXACT, ids=[e[0] for e in EXACT])
def test_exact_cases(rt, case):
    _, o, d, r, t_want, uv = case
    S = rt.pack_sweeps([o], [d], r)
    for res in (rt.sweep_spheres_bvh4(UNIT, None, S, brute_force=True), sc.product_sweep(S, UNIT)):
        if t_want is None:
            assert res[0][0] == np.inf and res[1][0] == sc.MISS and res[2][0] == 0 and res[3][0] == 0
        else:
            assert res[0][0] == f32(t_want) and res[1][0] == 0 and (res[2][0], res[3][0]) == (f32(uv[0]), f32(uv[1])), res


def test_items_that_are_not_walked(rt):
    tris = xc.geometry(rt, "tetra")
    nan = np.nan
    S = rt.pack_sweeps([[0, 0, 3]] * 8, [[0, 0, -1]] * 8, 0.25)
    S[1, 0] = nan; S[2, 5] = nan; S[3, 3] = nan; S[4, 3] = 0.0; S[5, 7] = -0.5; S[6, 4:7] = 0.0; S[7, 7] = nan
    res = rt.sweep_spheres_bvh4(tris, None, S, brute_force=True)
    assert res[1][0] != sc.MISS and np.isfinite(res[0][0])
    assert np.all(res[1][1:] == sc.MISS) and np.all(np.isinf(res[0][1:])) and np.all(res[2][1:] == 0) and np.all(res[3][1:] == 0)
    # radius 0 is a moving point, and t is in units of the direction: twice the length, half the time
    S0 = rt.pack_sweeps([[0.2, -0.1, 3]] * 2, [[0, 0, -1], [0, 0, -2]], 0.0)
    ray = rt.sweep_spheres_bvh4(tris, None, S0, brute_force=True)
    assert ray[1][0] != sc.MISS and ray[1][1] == ray[1][0] and abs(float(ray[0][1]) * 2 - float(ray[0][0])) < 1e-6


def _comb_sweeps(rt, n, seed):
    rng = np.random.default_rng(seed)
    org = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.9, 0.9, n), np.full(n, 2.0)], axis=1).astype(f32)
    d = np.stack([rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n), np.full(n, -1.0)], axis=1).astype(f32)
    return rt.pack_sweeps(org, d, rng.choice([0.0, 0.01, 0.05], n).astype(f32))


@pytest.mark.parametrize("all_hit", [True, False])
def test_comb_overruns_the_cap(rt, all_hit):
    """Pushes are dropped: the walk may miss the first contact, but what it returns is never earlier than brute force's, and the drops are
    counted."""
    tris, b4 = comb_bvh4(xc.COMB_LEVELS, xc.COMB_SEED, all_hit=all_hit)
    S = _comb_sweeps(rt, 512, 3)
    brute = rt.sweep_spheres_bvh4(tris, None, S, brute_force=True)
    res = rt.sweep_spheres_bvh4(tris, b4, S, stats=True)
    if all_hit:
        assert res[4]["stack_drops"] > 0 and res[4]["max_stack"] == 64, res[4]
        assert np.all(res[0] >= brute[0]) and np.any(res[0] > brute[0])
    else:                                                                                 # the sparse comb stays below the cap: exact
        assert res[4]["stack_drops"] == 0 and res[4]["max_stack"] < 64, res[4]
        sc.check_same_minimum(S, tris, res[:4], brute)
    sc.check_uv(S, tris, res[:4])


def test_spoiled_tree(rt, orc):
    tris = xc.geometry(rt, "spoiled")
    b4 = xc.spoiled_tree(rt, orc, tris)
    S = sc.sweep_set(rt, tris, 1024, 5)
    brute = rt.sweep_spheres_bvh4(tris, None, S, brute_force=True)
    res = rt.sweep_spheres_bvh4(tris, b4, S, stats=True)
    assert res[4]["stack_drops"] == 0
    assert np.all(res[0] >= brute[0]) and np.any(res[0] > brute[0])                       # some triangles cannot be reached
    sc.check_uv(S, tris, res[:4])


def test_error_codes(rt, orc):
    tris = xc.geometry(rt, "soup1k")
    b4 = xc.host_trees(rt, orc, tris, 0)[1]
    S = sc.sweep_set(rt, tris, 16, 1)
    with pytest.raises(rt.PtError) as e:
        rt.sweep_spheres_bvh4(tris, b4[:-9], S)                                           # a short buffer
    assert e.value.code == PT_ERR_BAD_BVH
    bad = b4.copy(); bad[1 + 3] = 0xFFFFFFF0                                              # fine: an out-of-range child is skipped
    rt.sweep_spheres_bvh4(tris, bad, S)
    with pytest.raises(rt.PtError) as e:
        rt.sweep_spheres_bvh4(tris, None, S)                                              # no tree without brute force
    assert e.value.code == PT_ERR_INVALID_ARG
    out = np.zeros((16, 4), np.uint32)
    t = np.ascontiguousarray(tris, f32)
    args = lambda sw, o, flags: rt.lib.pt_sweep_spheres_bvh4(t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(t.size // 9),
                                                             b4.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(b4.size), sw, C.c_uint64(16),
                                                             C.c_uint32(flags), o, None)
    sp, op = S.ctypes.data_as(C.POINTER(rt.PtSweep)), out.ctypes.data_as(C.POINTER(rt.PtHit))
    assert args(sp, op, 0) == 0
    assert args(None, op, 0) == PT_ERR_INVALID_ARG and args(sp, None, 0) == PT_ERR_INVALID_ARG and args(sp, op, 8) == PT_ERR_INVALID_ARG
    assert C.sizeof(rt.PtSweep) == 32 and rt.pack_sweeps([[0, 0, 0]], [[1, 0, 0]], 0.5, 2.0).tolist() == [[0, 0, 0, 2, 1, 0, 0, 0.5]]


@pytest.mark.parametrize("name,n", [("torus", 4096), ("dragon50k", 2048)])
def test_walk_equals_brute_force_on_many_sweeps(rt, orc, name, n):
    """Twin against twin needs no float64 reference: thousands of sweeps on the larger scenes, levels 0 and 2 and the refitted tree."""
    base = xc.geometry(rt, name)
    for label, tris, b4 in xc.forest(rt, orc, base):
        if label == "accel1":
            continue
        S = sc.sweep_set(rt, tris, n, 31)
        brute = rt.sweep_spheres_bvh4(tris, None, S, brute_force=True)
        res = rt.sweep_spheres_bvh4(tris, b4, S, stats=True)
        assert res[4]["stack_drops"] == 0, (label, res[4])
        sc.check_same_minimum(S, tris, res[:4], brute)
        sc.check_uv(S, tris, res[:4])


def test_the_callers_packed_records_are_not_written(rt, orc):
    """radius= and t_max= on packed (n, 8) records work on a copy: what pack_sweeps returned keeps its bits."""
    tris = xc.geometry(rt, "soup1k")
    b4 = xc.host_trees(rt, orc, tris, 0)[1]
    S = sc.sweep_set(rt, tris, 256, 2)
    keep = S.copy()
    want = rt.sweep_spheres_bvh4(tris, None, rt.pack_sweeps(S[:, 0:3], S[:, 4:7], 0.125, 2.0), brute_force=True)
    got = rt.sweep_spheres_bvh4(tris, None, S, radius=0.125, t_max=2.0, brute_force=True)
    assert sc.same_bits(S, keep)
    assert all(sc.same_bits(a, b) for a, b in zip(got, want))
    assert not sc.same_bits(got[0], rt.sweep_spheres_bvh4(tris, None, S, brute_force=True)[0])      # the override took effect
    rt.sweep_spheres_bvh4(tris, b4, S, radius=0.5)
    rt.sweep_spheres_bvh4(tris, b4, S[:, :], radius=S[:, 7] * 2)                          # a view of the records
    assert sc.same_bits(S, keep)


def test_a_contact_at_time_zero_ends_the_walk(rt, orc):
    """Behind t = 0 nothing can be accepted (t_T >= 0, strictly below best): the first leaf that overlaps at the start is the last one
    tested, where a walk that went on would test every triangle whose grown box holds the origin -- all of them for a sphere of four scene
    extents.  t and prim are those of brute force's first triangle at 0 in visit order all the same."""
    tris = xc.geometry(rt, "torus")
    b4 = xc.host_trees(rt, orc, tris, 0)[1]
    S = rt.pack_sweeps([[0.1, 0.2, 0.3]], [[1, 0, 0]], 4 * sc.extent_of(tris))
    res = rt.sweep_spheres_bvh4(tris, b4, S, stats=True)
    assert res[0][0] == 0 and res[1][0] != sc.MISS and not np.signbit(res[0][0])
    assert res[4]["tris_tested"] == 1 and res[4]["nodes_examined"] <= 4 * res[4]["max_stack"] + 1, res[4]
    brute = rt.sweep_spheres_bvh4(tris, None, S, brute_force=True, stats=True)
    assert brute[0][0] == 0 and brute[1][0] == 0 and brute[4]["tris_tested"] == tris.size // 9      # brute force tests every record
